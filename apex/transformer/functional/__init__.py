"""apex.transformer.functional — fused scale / mask / softmax, fused rotary position embedding and the
fused SwiGLU (``bias_swiglu``, from apex.ops.fused)."""
from ...ops.fused import bias_swiglu
from .fused_rope import (RotaryEmbedding, apply_rotary_qkv_grouped, apply_rotary_qkv_packed,
                         fused_apply_rotary_pos_emb, fused_apply_rotary_pos_emb_cached,
                         fused_apply_rotary_pos_emb_thd)
from .fused_softmax import FusedScaleMaskSoftmax, ScaledMaskedSoftmax, ScaledSoftmax, ScaledUpperTriangMaskedSoftmax
