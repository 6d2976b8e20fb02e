from .ms_deform_attn_func import MSDeformAttnFunction, MSDeformAttnFusedFunction, MSDeformAttnMixedFunction  # noqa: F401
