from .ms_deform_attn_func import (MSDeformAttnExactFunction, MSDeformAttnFunction, MSDeformAttnFusedFunction,  # noqa: F401
                                  MSDeformAttnMixedFunction, MSDeformAttnMixedFusedFunction)
