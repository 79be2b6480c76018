"""Fused rotary position embedding (apex.transformer.functional.fused_rope) over csrc/rope.hip.

Upstream-compatible entry points (non-interleaved "rotate half" pairing):

* ``fused_apply_rotary_pos_emb(t[s, b, h, d], freqs[s, 1, 1, d2], transpose_output_memory=False)``
* ``fused_apply_rotary_pos_emb_cached(t[s, b, h, d], cos_[s, 1, 1, d2], sin_[s, 1, 1, d2], ...)``
* ``fused_apply_rotary_pos_emb_thd(t[T, h, d], cu_seqlens, freqs[max_s, 1, 1, d2])``
* ``RotaryEmbedding(dim, rotary_percent, rotary_base, seq_len_interpolation_factor)``

and the project-native ``apply_rotary_qkv_packed(qkv[B, S, 3, h, d], cos[S, d2], sin[S, d2])`` the
GPT models call between the QKV projection and the packed flash attention: one launch rotates Q
and K and copies V into a new packed tensor; ``apply_rotary_qkv_grouped(qkv[B, S, H + 2 Hk, d], cos,
sin, H, Hk)`` is its grouped-query form (Q heads, then K heads, then V heads on one head axis).

One stride-generic kernel serves all of them: the tensor is handed over as an ``[S, B, H, D]`` view
(any seq / batch / head strides, D contiguous), the rotation is read from fp32-computed cos / sin
tables, the math is fp32 and the output is rounded once. The first ``d2`` elements of every head
are rotated, the rest copied. Backward is the same kernel applying the transposed rotation; only
the tables (and ``cu_seqlens``) are saved, never ``t``.

Dispatch follows apex._ext: device tensors require ``apex._C``; CPU tensors and
``APEX_FORCE_REFERENCE=1`` take :func:`rope_reference`, the PyTorch composition in this module that
is also the numerics reference of the tests. The device path takes fp32, bf16 and fp16; the
reference path additionally takes float64 (gradcheck). Anything else raises ``TypeError``.
"""
from __future__ import annotations

import torch

from ... import _ext

__all__ = ["fused_apply_rotary_pos_emb", "fused_apply_rotary_pos_emb_cached", "fused_apply_rotary_pos_emb_thd",
           "apply_rotary_qkv_packed", "apply_rotary_qkv_grouped", "RotaryEmbedding", "rope_reference",
           "rope_reference_qkv_packed", "rope_reference_qkv_grouped"]

_KERNEL_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


# ----------------------------------------------------------------------------------------------
# PyTorch reference composition (CPU path, APEX_FORCE_REFERENCE=1, tests' numerics reference)
# ----------------------------------------------------------------------------------------------
def _thd_rows(cu_seqlens, T, rows):
    """(table row, rotated?) of every token of a packed batch, without a host read of cu_seqlens."""
    cu = cu_seqlens.to(torch.int64)
    tok = torch.arange(T, device=cu.device)
    # largest j < nseq with cu[j] <= tok: empty sequences are stepped over
    j = torch.searchsorted(cu[1:].contiguous(), tok, right=True).clamp_(max=cu.numel() - 2)
    row = (tok - cu[j]).clamp_(0, rows - 1)
    return row, tok < cu[-1]


def _rotate(t4, cos, sin, rot_heads=None, cu_seqlens=None, backward=False):
    """The rotation on an [S, B, H, D] view, plain differentiable PyTorch. Math in fp32 (float64 for
    float64 input), one rounding to t's dtype."""
    S, B, H, D = t4.shape
    rows, d2 = cos.shape
    half = d2 // 2
    ct = torch.float64 if t4.dtype == torch.float64 else torch.float32
    live = None
    if cu_seqlens is not None:
        row, live = _thd_rows(cu_seqlens, S, rows)
        c, s = cos[row], sin[row]
    else:
        c, s = cos[:S], sin[:S]
    c, s = c.to(ct)[:, None, None, :], s.to(ct)[:, None, None, :]
    x = t4[..., :d2].to(ct)
    if backward:  # transpose of the map below
        g = x * s
        y = x * c + torch.cat([g[..., half:], -g[..., :half]], -1)
    else:
        y = x * c + torch.cat([-x[..., half:], x[..., :half]], -1) * s
    y = y.to(t4.dtype)
    if live is not None:
        y = torch.where(live[:, None, None, None], y, t4[..., :d2])
    if rot_heads is not None and rot_heads < H:
        y = torch.cat([y[:, :, :rot_heads], t4[:, :, rot_heads:, :d2]], 2)
    return torch.cat([y, t4[..., d2:]], -1) if d2 < D else y


def rope_reference(t, cos, sin, cu_seqlens=None):
    """Eager composition: ``t [s, b, h, d]`` (or ``[T, h, d]`` with ``cu_seqlens``) rotated by the
    ``[rows, d2]`` tables. Differentiable by autograd; the tests' and benchmarks' reference."""
    cos, sin = _tables(cos, sin)
    if cu_seqlens is not None:
        return _rotate(t.unsqueeze(1), cos, sin, cu_seqlens=cu_seqlens).squeeze(1)
    return _rotate(t, cos, sin)


def rope_reference_qkv_packed(qkv, cos, sin):
    """Eager composition of :func:`apply_rotary_qkv_packed`: Q and K rotated, V passed through."""
    cos, sin = _tables(cos, sin)
    B, S, three, h, d = qkv.shape
    t4 = qkv.reshape(B, S, 3 * h, d).transpose(0, 1)
    return _rotate(t4, cos, sin, rot_heads=2 * h).transpose(0, 1).reshape(B, S, 3, h, d)


def rope_reference_qkv_grouped(qkv, cos, sin, num_heads, num_kv_heads):
    """Eager composition of :func:`apply_rotary_qkv_grouped`: the Q and K heads rotated, V passed through."""
    _grouped_heads(qkv, num_heads, num_kv_heads)
    cos, sin = _tables(cos, sin)
    return _rotate(qkv.transpose(0, 1), cos, sin, rot_heads=num_heads + num_kv_heads).transpose(0, 1)


# ----------------------------------------------------------------------------------------------
# argument checks and the one launch site
# ----------------------------------------------------------------------------------------------
def _tables(cos, sin):
    """[rows, d2] views of tables given as [rows, d2] or [rows, 1, 1, d2]."""
    if cos.dim() == 4:
        cos, sin = cos.reshape(cos.shape[0], cos.shape[-1]), sin.reshape(sin.shape[0], sin.shape[-1])
    if cos.dim() != 2 or cos.shape != sin.shape:
        raise ValueError(f"cos / sin must both be [rows, d2] or [rows, 1, 1, d2], got {tuple(cos.shape)} and "
                         f"{tuple(sin.shape)}")
    return cos, sin


def _check(t4, cos, sin, dense):
    if not t4.is_floating_point() or (t4.dtype not in _KERNEL_DTYPES and t4.dtype != torch.float64):
        raise TypeError(f"fused rope supports fp32, bf16 and fp16 tensors, got {t4.dtype}")
    if not cos.is_floating_point():
        raise TypeError(f"rope tables must be floating point, got {cos.dtype}")
    rows, d2 = cos.shape
    if d2 % 2:
        raise ValueError(f"the rotary dimension must be even, got d2={d2}")
    if d2 > t4.shape[-1]:
        raise ValueError(f"the rotary dimension d2={d2} exceeds the head dimension {t4.shape[-1]}")
    if rows < 1 or (dense and rows < t4.shape[0]):
        raise ValueError(f"the cos / sin table has {rows} rows for a sequence of {t4.shape[0]}")


def _launch(t4, out4, cos, sin, cu_seqlens, rot_heads, backward):
    """out4 <- rotation of t4 (both [S, B, H, D] views); the native kernel or the reference."""
    if _ext.use_native(t4):
        if t4.dtype not in _KERNEL_DTYPES:
            raise TypeError(f"the fused rope kernel supports fp32, bf16 and fp16 tensors, got {t4.dtype}")
        if t4.shape[-1] > 1 and t4.stride(-1) != 1:
            t4 = t4.contiguous()
        if cos.dtype != torch.float32 and cos.dtype != t4.dtype:
            cos, sin = cos.float(), sin.float()
        cu = None
        if cu_seqlens is not None:
            cu = cu_seqlens if cu_seqlens.dtype == torch.int32 else cu_seqlens.to(torch.int32)
            cu = cu.contiguous()
        _ext.require().rope(t4, out4, cos.contiguous(), sin.contiguous(), cu,
                            -1 if rot_heads is None else rot_heads, backward)
    else:
        with torch.no_grad():
            out4.copy_(_rotate(t4, cos, sin, rot_heads, cu_seqlens, backward))
    return out4


def _empty_sbhd(t4, transpose_output_memory):
    S, B, H, D = t4.shape
    if transpose_output_memory:
        return t4.new_empty(B, S, H, D).transpose(0, 1)
    return t4.new_empty(S, B, H, D)


class _FusedRoPECached(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, cos, sin, transpose_output_memory):
        ctx.save_for_backward(cos, sin)
        ctx.transpose_output_memory = transpose_output_memory
        return _launch(t, _empty_sbhd(t, transpose_output_memory), cos, sin, None, None, False)

    @staticmethod
    def backward(ctx, dy):
        cos, sin = ctx.saved_tensors
        return _launch(dy, _empty_sbhd(dy, ctx.transpose_output_memory), cos, sin, None, None, True), None, None, None


class _FusedRoPETHD(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, cu_seqlens, cos, sin):
        ctx.save_for_backward(cu_seqlens, cos, sin)
        out = torch.empty(t.shape, dtype=t.dtype, device=t.device)
        _launch(t.unsqueeze(1), out.unsqueeze(1), cos, sin, cu_seqlens, None, False)
        return out

    @staticmethod
    def backward(ctx, dy):
        cu_seqlens, cos, sin = ctx.saved_tensors
        dx = torch.empty(dy.shape, dtype=dy.dtype, device=dy.device)
        _launch(dy.unsqueeze(1), dx.unsqueeze(1), cos, sin, cu_seqlens, None, True)
        return dx, None, None, None


class _FusedRoPEQKVPacked(torch.autograd.Function):
    """Packed QKV, ``[B, S, 3, h, d]`` or grouped ``[B, S, heads, d]``: the first ``rot_heads`` heads of
    the flattened head axis are rotated, the rest (V) copied."""

    @staticmethod
    def _run(x, cos, sin, rot_heads, backward):
        B, S, d = x.shape[0], x.shape[1], x.shape[-1]
        # a packed (3, h) pair must flatten to one head axis
        if x.stride(-1) != 1 or (x.dim() == 5 and x.stride(2) != x.shape[3] * x.stride(3)):
            x = x.contiguous()
        heads = x.shape[2] * x.shape[3] if x.dim() == 5 else x.shape[2]
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        x4 = x.as_strided((S, B, heads, d), (x.stride(1), x.stride(0), x.stride(-2), 1), x.storage_offset())
        _launch(x4, out.view(B, S, heads, d).transpose(0, 1), cos, sin, None, rot_heads, backward)
        return out

    @staticmethod
    def forward(ctx, qkv, cos, sin, rot_heads):
        ctx.save_for_backward(cos, sin)
        ctx.rot_heads = rot_heads
        return _FusedRoPEQKVPacked._run(qkv, cos, sin, rot_heads, False)

    @staticmethod
    def backward(ctx, dy):
        # out of place: the incoming gradient may be shared with other consumers; dV is copied
        cos, sin = ctx.saved_tensors
        return _FusedRoPEQKVPacked._run(dy, cos, sin, ctx.rot_heads, True), None, None, None


# ----------------------------------------------------------------------------------------------
# public entry points
# ----------------------------------------------------------------------------------------------
def fused_apply_rotary_pos_emb_cached(t, cos_, sin_, transpose_output_memory=False):
    """Rotate ``t [s, b, h, d]`` by precomputed tables ``cos_ / sin_ [s, 1, 1, d2]`` (or ``[s, d2]``),
    fp32 or ``t``'s dtype. With ``transpose_output_memory`` the result is an ``[s, b, h, d]`` view of
    ``[b, s, h, d]`` memory. No gradient flows to the tables."""
    if t.dim() != 4:
        raise ValueError(f"t must be [s, b, h, d], got {tuple(t.shape)}")
    cos, sin = _tables(cos_, sin_)
    _check(t, cos, sin, dense=True)
    return _FusedRoPECached.apply(t, cos.detach(), sin.detach(), bool(transpose_output_memory))


def fused_apply_rotary_pos_emb(t, freqs, transpose_output_memory=False):
    """Rotate ``t [s, b, h, d]`` by the angles ``freqs [s, 1, 1, d2]`` (fp32). The cos / sin tables are
    built once per call in fp32 and handed to the cached path."""
    f = freqs.detach().float()
    return fused_apply_rotary_pos_emb_cached(t, torch.cos(f), torch.sin(f), transpose_output_memory)


def fused_apply_rotary_pos_emb_thd(t, cu_seqlens, freqs):
    """Rotate packed sequences ``t [T, h, d]``: token ``k`` of sequence ``j`` (``cu_seqlens[j] + k``) is
    rotated by row ``k`` of ``freqs [max_s, 1, 1, d2]``; tokens at or past ``cu_seqlens[-1]`` are
    copied. ``cu_seqlens`` (int32, on ``t``'s device) is only ever read on the device."""
    if t.dim() != 3:
        raise ValueError(f"t must be [T, h, d], got {tuple(t.shape)}")
    if cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2 or cu_seqlens.is_floating_point():
        raise ValueError("cu_seqlens must be an integer vector [num_sequences + 1]")
    f = freqs.detach().float()
    cos, sin = _tables(torch.cos(f), torch.sin(f))
    _check(t.unsqueeze(1), cos, sin, dense=False)
    return _FusedRoPETHD.apply(t, cu_seqlens, cos, sin)


def apply_rotary_qkv_packed(qkv, cos, sin):
    """Rotate the Q and K thirds of packed ``qkv [B, S, 3, h, d]`` by the ``[S, d2]`` tables and copy V,
    in one launch, into a new packed tensor (out of place; so is the backward)."""
    if qkv.dim() != 5 or qkv.shape[2] != 3:
        raise ValueError(f"qkv must be [B, S, 3, h, d], got {tuple(qkv.shape)}")
    cos, sin = _tables(cos, sin)
    _check(qkv.transpose(0, 1), cos, sin, dense=True)
    return _FusedRoPEQKVPacked.apply(qkv, cos.detach(), sin.detach(), 2 * qkv.shape[3])


def _grouped_heads(qkv, num_heads, num_kv_heads):
    if qkv.dim() != 4 or num_kv_heads < 1 or num_heads % num_kv_heads or \
            qkv.shape[2] != num_heads + 2 * num_kv_heads:
        raise ValueError(f"qkv must be [B, S, num_heads + 2 * num_kv_heads, d] with num_heads a multiple of "
                         f"num_kv_heads, got {tuple(qkv.shape)} for {num_heads} / {num_kv_heads} heads")


def apply_rotary_qkv_grouped(qkv, cos, sin, num_heads, num_kv_heads):
    """Grouped-query form of :func:`apply_rotary_qkv_packed`: ``qkv [B, S, H + 2 Hk, d]`` holds the ``H``
    query heads, then the ``Hk`` key heads, then the ``Hk`` value heads. Heads ``[0, H + Hk)`` are
    rotated by the ``[S, d2]`` tables and the V heads copied, in one launch, into a new tensor of the
    same layout (out of place; so is the backward)."""
    _grouped_heads(qkv, num_heads, num_kv_heads)
    cos, sin = _tables(cos, sin)
    _check(qkv.transpose(0, 1), cos, sin, dense=True)
    return _FusedRoPEQKVPacked.apply(qkv, cos.detach(), sin.detach(), num_heads + num_kv_heads)


class RotaryEmbedding(torch.nn.Module):
    """Rotary angles and their cos / sin tables.

    ``forward(max_seq_len, offset=0)`` returns the fp32 angles ``[max_seq_len, 1, 1, dim]``
    (``cat(outer(pos, inv_freq),) x 2``), ``cos_sin(max_seq_len, offset=0)`` the fp32 ``[max_seq_len,
    dim]`` tables. ``dim`` is ``int(dim * rotary_percent)``. Frequencies and tables are plain
    attributes, not buffers: ``module.to(torch.bfloat16)`` and amp O2 leave them in fp32 (bf16 angles
    at position 1e5 are garbage) and they never appear in ``state_dict()``. They are rebuilt when the
    length, offset or device changes.
    """

    def __init__(self, dim, rotary_percent=1.0, rotary_base=10000, seq_len_interpolation_factor=None):
        super().__init__()
        if rotary_percent < 1.0:
            dim = int(dim * rotary_percent)
        if dim < 2 or dim % 2:
            raise ValueError(f"the rotary dimension must be even and positive, got {dim}")
        self.dim = dim
        self.seq_len_interpolation_factor = seq_len_interpolation_factor
        self.inv_freq = 1.0 / (rotary_base ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim))
        self._key = None
        self._freqs = self._cos = self._sin = None

    def _build(self, max_seq_len, offset, device):
        device = torch.device(device) if device is not None else self.inv_freq.device
        key = (int(max_seq_len), int(offset), device)
        if key != self._key:
            if self.inv_freq.device != device:
                self.inv_freq = self.inv_freq.to(device)
            seq = torch.arange(max_seq_len, device=device, dtype=torch.float32) + offset
            if self.seq_len_interpolation_factor is not None:
                seq = seq * (1.0 / self.seq_len_interpolation_factor)
            freqs = torch.outer(seq, self.inv_freq)
            self._freqs = torch.cat((freqs, freqs), dim=-1)
            self._cos, self._sin = torch.cos(self._freqs), torch.sin(self._freqs)
            self._key = key

    def forward(self, max_seq_len, offset=0, device=None):
        self._build(max_seq_len, offset, device)
        return self._freqs[:, None, None, :]

    def cos_sin(self, max_seq_len, offset=0, device=None):
        self._build(max_seq_len, offset, device)
        return self._cos, self._sin
