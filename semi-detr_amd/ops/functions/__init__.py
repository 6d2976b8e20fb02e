from .ms_deform_attn_func import MSDeformAttnFunction, MSDeformAttnFusedFunction, MSDeformAttnMixedFunction, MSDeformAttnMixedFusedFunction  # noqa: F401
