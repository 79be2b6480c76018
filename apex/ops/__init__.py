"""apex.ops — functional fused ops (HIP kernels with PyTorch reference formulations)."""
from . import fused  # noqa: F401
from .fused import (ACT_GELU, ACT_GELU_TANH, ACT_SILU, bias_geglu, bias_swiglu, gated_act,  # noqa: F401
                    gated_act_reference)
from . import grouped  # noqa: F401
from .grouped import (Routing, grouped_gemm_supported, grouped_linear, moe_permute, moe_route,  # noqa: F401
                      moe_route_supported, moe_unpermute)
