from .ms_deform_attn import MSDeformAttn, convert_exact_backward  # noqa: F401
