"""apex.ops — functional fused ops (HIP kernels with PyTorch reference formulations)."""
from . import fused  # noqa: F401
from .fused import (ACT_GELU, ACT_GELU_TANH, ACT_SILU, bias_geglu, bias_swiglu, gated_act,  # noqa: F401
                    gated_act_reference)
