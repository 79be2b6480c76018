"""Attention core used by apex.contrib.multihead_attn and the model zoo (NS-05).

``attention_packed(qkv[B,S,3,h,d], bias, p, causal, scale, k_lens) -> [B,S,h,d]`` and
``attention(q, k, v, ...)`` for separate [B, S, h, d] views. Grouped-query attention: ``attention``
takes k / v with hk < h heads (h % hk == 0), and ``attention_grouped_packed(qkv[B,S,h+2hk,d], h, hk,
...)`` the packed projection output (query heads, then key heads, then value heads); the flash
kernels read each K/V head once per query head of its group, nothing is expanded.

Every bf16/fp16 device call runs the MFMA flash-attention kernels in apex._C
(csrc/attention_fwd.h, csrc/attention_bwd.h; launchers in csrc/attention_impl.h):

* head dims 32 / 64 / 128 / 256 natively; any other head dim up to 256 (multiple of 8) is
  zero-padded to the next of those (zero columns add nothing to Q K^T, and the padded V columns
  are sliced off the output), with the softmax scale of the ORIGINAL head dim;
* ``attn_bias``: an additive score bias broadcastable to [B, h, Sq, Sk] (attention masks as
  -inf, ALiBi, relative-position biases) is added inside the kernel — no [B, h, Sq, Sk] score
  tensor is materialised; a boolean mask follows scaled_dot_product_attention's convention
  (True = attend) and becomes a 0 / -inf bias. A bias that requires a gradient gets it from the
  backward kernels: dS written into an fp32 tensor of the bias's (broadcast) shape, atomically
  added over the broadcast dims;
* ``k_lens``: per-batch valid key lengths (right padding) skip whole key tiles.

fp32 device inputs (head dims up to 128) run the f32-MFMA flash kernels (csrc/attention_f32.hip:
exact f32 products and accumulation, the same masks / bias / dropout semantics).

Device calls the flash kernels do not take — fp32 head dims > 128, head dims > 256 — run the
query-blocked memory-efficient path (``chunked.chunked_attention``: O(S * block) memory, backward by
recomputation from the saved log-sum-exp, bias gradient = the score gradient), never the O(S^2)
composition. The reference composition (``attention_reference``: matmul -> softmax in fp32 ->
dropout -> matmul) runs on CPU tensors; ``APEX_ATTN_BACKEND=reference`` forces it (A/B, numerics
checks).
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn.functional as F

from ... import _ext

_NATIVE_DIMS = (32, 64, 128, 256)


def _padded_dim(d):
    for n in _NATIVE_DIMS:
        if d <= n:
            return n
    return None


def _native_ok(t, bias):
    if os.environ.get("APEX_ATTN_BACKEND", "native") in ("reference", "sdpa", "chunked"):
        return False
    if not t.is_cuda:
        return False
    d = t.shape[-1]
    if d % 8 or _padded_dim(d) is None:
        return False
    if t.dtype == torch.float32:
        # fp32: the f32-MFMA kernels (csrc/attention_f32.hip), head dims up to 128;
        # APEX_ATTN_F32=0 selects the torch compositions (A/B)
        if os.environ.get("APEX_ATTN_F32", "1") == "0" or _padded_dim(d) > 128:
            return False
    elif t.dtype not in (torch.float16, torch.bfloat16):
        return False
    C = _ext._load()
    return C is not None and hasattr(C, "flash_attn_fwd")


def prepare_bias(bias, B, H, Sq, Sk, dtype):
    """An additive bias as a [B|1, H|1, Sq|1, Sk] view in ``dtype`` whose rows the kernel can load
    8 bytes at a time (key-contiguous, row stride a multiple of 4 elements). Broadcast dims keep
    size 1; nothing is expanded to the full score shape."""
    if bias is None:
        return None
    if bias.dtype == torch.bool:
        bias = torch.zeros(bias.shape, dtype=dtype, device=bias.device).masked_fill(~bias, float("-inf"))
    # (no detach: a trainable bias keeps its graph; the flash backward returns dS for this view)
    bias = bias.to(dtype)
    while bias.dim() < 4:
        bias = bias.unsqueeze(0)
    if bias.shape[-1] != Sk:
        bias = bias.expand(*bias.shape[:-1], Sk)
    for dim, full in zip(range(3), (B, H, Sq)):
        if bias.shape[dim] not in (1, full):
            raise ValueError(f"attention bias of shape {tuple(bias.shape)} does not broadcast to "
                             f"[{B}, {H}, {Sq}, {Sk}]")
    ok = bias.stride(-1) == 1 and all(bias.stride(i) % 4 == 0 or bias.shape[i] == 1 for i in range(3)) and \
        bias.data_ptr() % (16 if dtype == torch.float32 else 8) == 0
    if not ok:
        sk4 = (Sk + 3) // 4 * 4
        buf = torch.zeros(*bias.shape[:-1], sk4, dtype=dtype, device=bias.device)
        buf[..., :Sk] = bias
        bias = buf[..., :Sk]
    return bias


def attention_reference(q, k, v, attn_bias=None, dropout_p=0.0, causal=False, scale=None, k_lens=None):
    """q: [B, Sq, h, d], k/v: [B, Sk, h, d] -> [B, Sq, h, d] (fp32 softmax statistics). k / v with
    hk < h heads (grouped-query attention) are expanded group-wise first."""
    B, Sq, H, d = q.shape
    k, v = _expand_kv(q, k, v)
    Sk = k.shape[1]
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) * scale
    if attn_bias is not None:
        bias = attn_bias
        if bias.dtype == torch.bool:
            bias = torch.zeros(bias.shape, device=bias.device).masked_fill(~bias, float("-inf"))
        s = s + bias.float()
    if k_lens is not None:
        km = torch.arange(Sk, device=q.device)[None, :] >= k_lens[:, None].long()
        s = s.masked_fill(km[:, None, None, :], float("-inf"))
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    p = torch.softmax(s, -1).nan_to_num(0.0)  # fully masked rows -> 0, as the kernels do
    if dropout_p > 0:
        p = F.dropout(p, dropout_p, True)
    return torch.einsum("bhqk,bkhd->bqhd", p, v.float()).to(q.dtype)


def _check_groups(H, Hk):
    if Hk != H and (Hk < 1 or H % Hk):
        raise ValueError(f"grouped-query attention needs the {H} query heads to be a multiple of the "
                         f"{Hk} key/value heads")


def _expand_kv(q, k, v):
    """Grouped-query K/V ([B, Sk, hk, d], hk a divisor of q's h) expanded to one head per query head,
    for the paths that do not reach the flash kernels; autograd sums the gradient over each group."""
    H, Hk = q.shape[2], k.shape[2]
    _check_groups(H, Hk)
    if Hk == H:
        return k, v
    g = H // Hk
    return k.repeat_interleave(g, dim=2), v.repeat_interleave(g, dim=2)


def _pad_last(t, n):
    return F.pad(t, (0, n - t.shape[-1])) if t.shape[-1] != n else t


def _kernel_view(t):
    """``t`` as the flash binding takes it: last dim contiguous, every other stride a multiple of 8
    elements, 16-byte aligned. Any other view (a slice that starts off a 16-byte boundary, a head dim
    cut out of a wider one) is copied to a contiguous tensor, as apex.ops.fused's ``_wgrad`` does for an
    unaligned slot; the copy is differentiable, so the gradient still reaches the view."""
    ok = t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:-1]) and t.data_ptr() % 16 == 0
    return t if ok else t.clone(memory_format=torch.contiguous_format)


def _kernel_k_lens(k_lens, device):
    """Key lengths as the kernels read them: a contiguous int32 tensor on the operands' device."""
    if k_lens is None:
        return None
    return torch.as_tensor(k_lens).to(device=device, dtype=torch.int32).contiguous()


def attention_packed(qkv, attn_bias=None, dropout_p=0.0, causal=False, scale=None, k_lens=None):
    B, S, three, h, d = qkv.shape
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    if _native_ok(qkv, attn_bias):
        from . import flash

        bias = prepare_bias(attn_bias, B, h, S, S, qkv.dtype)
        k_lens = _kernel_k_lens(k_lens, qkv.device)
        dp = _padded_dim(d)
        if dp == d:
            return flash.flash_attention_packed(_kernel_view(qkv), dropout_p, causal, scale, k_lens, bias)
        o = flash.flash_attention_packed(_pad_last(qkv, dp), dropout_p, causal, scale, k_lens, bias)
        return o[..., :d]
    q, k, v = qkv.unbind(2)
    return _fallback(q, k, v, attn_bias, dropout_p, causal, scale, k_lens)


def _short_dense_ok(q, k, attn_bias):
    """Training-length fp32 attention (S <= 1024, fp32 scores of at most 2 GiB, no trainable bias):
    the dense composition — one fused softmax and one fused dropout kernel each way, probabilities
    kept for backward — beats the query-blocked path's recomputation (~3x the elementwise passes
    over [B, h, S, S]): the fp32 BERT-Large step (the bench's speedup denominator, micro-batch 256)
    1741 ms blocked vs 1567 ms dense (BENCH_r02). Longer sequences keep O(S * block) memory."""
    B, Sq, H, _ = q.shape
    Sk = k.shape[1]
    trainable = attn_bias is not None and attn_bias.requires_grad and torch.is_grad_enabled()
    return Sq <= 1024 and Sk <= 1024 and B * H * Sq * Sk * 4 <= (2 << 30) and not trainable


def _fallback(q, k, v, attn_bias, dropout_p, causal, scale, k_lens):
    backend = os.environ.get("APEX_ATTN_BACKEND", "native")
    if q.is_cuda and backend != "reference" and not (backend != "chunked" and _short_dense_ok(q, k, attn_bias)):
        from .chunked import chunked_attention

        return chunked_attention(q, k, v, attn_bias, dropout_p, causal, scale, k_lens)
    return attention_reference(q, k, v, attn_bias, dropout_p, causal, scale, k_lens)


def attention_grouped_packed(qkv, num_heads, num_kv_heads, attn_bias=None, dropout_p=0.0, causal=False,
                             scale=None, k_lens=None):
    """Grouped-query attention on the packed projection output ``qkv [B, S, H + 2 Hk, d]`` (the H query
    heads, then the Hk key heads, then the Hk value heads) -> [B, S, H, d]."""
    H, Hk = int(num_heads), int(num_kv_heads)
    _check_groups(H, Hk)
    if qkv.dim() != 4 or qkv.shape[2] != H + 2 * Hk:
        raise ValueError(f"qkv must be [B, S, num_heads + 2 * num_kv_heads, d], got {tuple(qkv.shape)} for "
                         f"{H} / {Hk} heads")
    B, S, _, d = qkv.shape
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    if _native_ok(qkv, attn_bias):
        from . import flash

        bias = prepare_bias(attn_bias, B, H, S, S, qkv.dtype)
        k_lens = _kernel_k_lens(k_lens, qkv.device)
        dp = _padded_dim(d)
        if dp == d:
            return flash.flash_attention_grouped_packed(_kernel_view(qkv), H, Hk, dropout_p, causal, scale, k_lens, bias)
        o = flash.flash_attention_grouped_packed(_pad_last(qkv, dp), H, Hk, dropout_p, causal, scale, k_lens, bias)
        return o[..., :d]
    q, k, v = qkv[:, :, :H], qkv[:, :, H:H + Hk], qkv[:, :, H + Hk:]
    k, v = _expand_kv(q, k, v)
    return _fallback(q, k, v, attn_bias, dropout_p, causal, scale, k_lens)


def attention(q, k, v, attn_bias=None, dropout_p=0.0, causal=False, scale=None, k_lens=None):
    """q: [B, Sq, h, d], k/v: [B, Sk, hk, d] -> [B, Sq, h, d]; hk == h, or a divisor of it for
    grouped-query attention (query heads [j h/hk, (j + 1) h/hk) attend to K/V head j)."""
    B, Sq, h, d = q.shape
    _check_groups(h, k.shape[2])
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    if _native_ok(q, attn_bias):
        from . import flash

        bias = prepare_bias(attn_bias, B, h, Sq, k.shape[1], q.dtype)
        k_lens = _kernel_k_lens(k_lens, q.device)
        dp = _padded_dim(d)
        if dp == d:
            return flash.flash_attention(_kernel_view(q), _kernel_view(k), _kernel_view(v), dropout_p, causal, scale,
                                         k_lens, bias)
        o = flash.flash_attention(_pad_last(q, dp), _pad_last(k, dp), _pad_last(v, dp), dropout_p, causal, scale,
                                  k_lens, bias)
        return o[..., :d]
    k, v = _expand_kv(q, k, v)
    return _fallback(q, k, v, attn_bias, dropout_p, causal, scale, k_lens)
