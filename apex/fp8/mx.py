"""MXFP8: OCP Microscaling fp8 on gfx950's block-scaled MFMA, with the block scales in use.

Every 32 consecutive values along the contraction carry their own power-of-two scale (one E8M0
byte, 2^(s - 127)), computed from that block's own amax when it is quantised: no amax history, no
per-tensor state to checkpoint or all-reduce, and an outlier costs precision in its own block only.

  mx_quantize    x [R, C] -> (codes, scales) rowwise (blocks along C) and / or colwise (codes [C, R],
                 blocks along R), one launch (csrc/mx.hip)
  mx_gemm        C = (A . 2^(sa - 127)) (B . 2^(sb - 127))^T (+ bias), csrc/gemm_mx.hip
  mx_dequantize  the values a (codes, scales) pair encodes — torch, for debugging and fallbacks
  mx_supported   the shape predicate of mx_gemm; callers use it to decline, not to crash
  mx_linear      autograd linear layer whose three GEMMs run on mx_gemm; ``MXLinear`` wraps it

Scale byte of a block: ``s = max(E - emax, 0)`` with E the biased fp32 exponent of the block's amax
and emax = 8 (e4m3) / 15 (e5m2); codes = sat(x * 2^(127 - s)) rounded to nearest even. A block that
holds an inf or a NaN gets ``s = 0xFF`` (the E8M0 NaN) and is converted unscaled the way the
per-tensor quantisers convert non-finite values (+-inf -> +-max, NaN -> -max).

CPU tensors and ``APEX_FORCE_REFERENCE=1`` take a torch path with the same contract.
Nothing in ``Fp8Recipe`` / ``fp8_autocast`` routes to these functions: they are called directly.
"""
from __future__ import annotations

import torch

from .. import _ext
from . import _FMT_NAMES, E4M3, E5M2, FMT_MAX, _aligned, _C

__all__ = ["mx_quantize", "mx_dequantize", "mx_gemm", "mx_supported", "mx_linear", "MXLinear"]

_EMAX = {E4M3: 8, E5M2: 15}
_F8T = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}
_IN_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _fmt(f):
    f = _FMT_NAMES.get(f, f) if isinstance(f, str) else f
    if f not in (E4M3, E5M2):
        raise ValueError(f"mx: format {f!r}: expected E4M3 / E5M2 (or 'e4m3' / 'e5m2')")
    return f


def _ref_quantize_rows(x, fmt):
    """The contract in fp32 torch arithmetic: x [R, C] -> codes [R, C], scales [R, C / 32]."""
    R, C = x.shape
    xb = x.float().reshape(R, C // 32, 32)
    E = (xb.contiguous().view(torch.int32) & 0x7FFFFFFF).amax(dim=-1) >> 23
    bad = E == 255
    s = torch.where(bad, torch.full_like(E, 255), (E - _EMAX[fmt]).clamp(min=0))
    mult = torch.ldexp(torch.ones_like(s, dtype=torch.float32), torch.where(bad, torch.zeros_like(s), 127 - s))
    p = xb * mult.unsqueeze(-1)  # exact: a power of two
    p = torch.where(torch.isnan(p), torch.full_like(p, -FMT_MAX[fmt]), p).clamp(-FMT_MAX[fmt], FMT_MAX[fmt])
    return p.to(_F8T[fmt]).view(torch.uint8).reshape(R, C), s.to(torch.uint8)


def mx_quantize(x, fmt=E4M3, rowwise=True, colwise=False):
    """x [R, C] (bf16 / fp16 / fp32) -> MX operands, one ``(codes, scales)`` pair per requested
    orientation (the pair itself when one is requested, ``(rowwise pair, colwise pair)`` for both),
    all from one launch that reads x once.
      rowwise  codes [R, C], scales [R, C / 32]; needs C % 32 == 0
      colwise  codes [C, R], scales [C, R / 32] (the transposed codes, blocks along R); R % 32 == 0
    """
    fmt = _fmt(fmt)
    if x.dim() != 2 or x.dtype not in _IN_DTYPES:
        raise ValueError("mx_quantize: a 2-D bf16 / fp16 / fp32 tensor")
    R, C = x.shape
    if not (rowwise or colwise) or R < 1 or C < 1 or (rowwise and C % 32) or (colwise and R % 32):
        raise ValueError(f"mx_quantize: shape {tuple(x.shape)}: rowwise needs C % 32 == 0, colwise R % 32 == 0")
    if _ext.use_native(x):
        out = _C().mx_quantize(_aligned(x.detach()), fmt, rowwise, colwise)
        pairs = [(out[i], out[i + 1]) for i in range(0, len(out), 2)]
    else:
        pairs = ([_ref_quantize_rows(x.detach(), fmt)] if rowwise else []) + \
                ([_ref_quantize_rows(x.detach().t(), fmt)] if colwise else [])
    return pairs[0] if len(pairs) == 1 else tuple(pairs)


def mx_dequantize(codes, scales, fmt, dtype=torch.float32):
    """(codes [R, K], scales [R, K / 32]) -> the encoded values in ``dtype`` (a 0xFF scale: NaN)."""
    fmt = _fmt(fmt)
    s = scales.to(torch.int32)
    f = torch.ldexp(torch.ones_like(s, dtype=torch.float32), s - 127)
    f = torch.where(s == 255, torch.full_like(f, float("nan")), f)
    return (codes.view(_F8T[fmt]).to(torch.float32) * f.repeat_interleave(32, dim=1)).to(dtype)


def mx_supported(M, K, N, native=True):
    """Can ``mx_gemm`` take a [M, K] x [N, K]^T product? The kernel (``native``, device tensors) needs
    K % 128 == 0 and N % 8 == 0 (its operands must also be contiguous and 16-byte aligned, which
    ``mx_quantize`` outputs are); the torch reference path only whole blocks, K % 32 == 0."""
    if not native:
        return M >= 1 and N >= 1 and K >= 32 and K % 32 == 0
    return M >= 1 and K >= 128 and K % 128 == 0 and N >= 8 and N % 8 == 0 and max(M, N, K) < 2 ** 31 - 256


def mx_gemm(a, a_scales, b, b_scales, fmt_a=E4M3, fmt_b=E4M3, bias=None, out_dtype=torch.bfloat16):
    """C [M, N] = (a . 2^(a_scales - 127)) (b . 2^(b_scales - 127))^T (+ bias) in ``out_dtype`` (bf16 /
    fp16 / fp32) from an fp32 accumulator. a [M, K], b [N, K]: uint8 codes in ``fmt_a`` / ``fmt_b``;
    scales [M, K / 32], [N, K / 32]: E8M0 bytes; K % 128 == 0, N % 8 == 0 (``mx_supported``), all
    contiguous and 16-byte aligned. There is no alpha: MX has no per-tensor factor.

    A 0xFF scale byte (what ``mx_quantize`` gives a block with an inf or a NaN) is the E8M0 NaN, and
    the MFMA honours it (measured on MI355X, pinned by tests/test_mx_gpu.py::test_nan_scale): every
    output element whose row of a or of b has such a block is NaN, whatever that block's codes —
    all-zero codes included — and no other element is touched. The torch path does the same."""
    fmt_a, fmt_b = _fmt(fmt_a), _fmt(fmt_b)
    M, K = a.shape
    N = b.shape[0]
    if not mx_supported(M, K, N, _ext.use_native(a)) or tuple(b.shape) != (N, K) or tuple(a_scales.shape) != (M, K // 32) or \
            tuple(b_scales.shape) != (N, K // 32):
        raise ValueError(f"mx_gemm: unsupported shapes a {tuple(a.shape)} / {tuple(a_scales.shape)}, "
                         f"b {tuple(b.shape)} / {tuple(b_scales.shape)} (K % 128 == 0, N % 8 == 0)")
    if bias is not None and bias.dtype != out_dtype:
        bias = bias.to(out_dtype)
    if _ext.use_native(a):
        return _C().gemm_mx(_aligned(a), _aligned(a_scales), _aligned(b), _aligned(b_scales), fmt_a, fmt_b,
                            None if bias is None else _aligned(bias.detach()), out_dtype)

    def val(codes, scales, fmt):  # float64 (0xFF: NaN, also times a zero code)
        s = scales.to(torch.int32)
        f = torch.ldexp(torch.ones(s.shape, dtype=torch.float64, device=s.device), s - 127)
        f = torch.where(s == 255, torch.full_like(f, float("nan")), f)
        return codes.view(_F8T[fmt]).to(torch.float64) * f.repeat_interleave(32, dim=1)

    c = (val(a, a_scales, fmt_a) @ val(b, b_scales, fmt_b).t()).float()
    if bias is not None:
        c = c + bias.float()
    return c.to(out_dtype)


class _MXLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, fwd, bwd):
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        M, N = x2.shape[0], weight.shape[0]
        # dW [N, K] = dy_col [N, M] . x_col [K, M]^T contracts over the M tokens: x's colwise codes are
        # made by the same launch as the forward operand and are what is kept for it
        wgrad = ctx.needs_input_grad[1] and mx_supported(N, M, K, _ext.use_native(x))
        if wgrad:
            (x8, xs), xcol = mx_quantize(x2, fwd, True, True)
        else:
            (x8, xs), xcol = mx_quantize(x2, fwd, True, False), None
        w8, ws = mx_quantize(weight, fwd, True, False)
        y = mx_gemm(x8, xs, w8, ws, fwd, fwd, bias, x.dtype)
        ctx.fmts, ctx.has_bias, ctx.wgrad, ctx.xshape = (fwd, bwd), bias is not None, wgrad, x.shape
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.save_for_backward(weight, *(xcol if wgrad else (x2,)))
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        fwd, bwd = ctx.fmts
        weight = ctx.saved_tensors[0]
        N, K = weight.shape
        dy2 = _aligned(dy.reshape(-1, N))
        M = dy2.shape[0]
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        # dx [M, K] = dy_row [M, N] . W_col [K, N]^T contracts over N
        dgrad = need_dx and mx_supported(M, N, K, _ext.use_native(dy))
        wgrad = need_dw and ctx.wgrad
        dyr = dyc = None
        if dgrad and wgrad:
            dyr, dyc = mx_quantize(dy2, bwd, True, True)
        elif dgrad:
            dyr = mx_quantize(dy2, bwd, True, False)
        elif wgrad:
            dyc = mx_quantize(dy2, bwd, False, True)
        dx = dw = db = None
        if dgrad:
            wc8, wcs = mx_quantize(weight, fwd, False, True)  # codes [K, N], blocks along N
            dx = mx_gemm(dyr[0], dyr[1], wc8, wcs, bwd, fwd, None, dy.dtype)
        elif need_dx:  # a contraction (N) the kernel declines
            dx = dy2 @ weight.to(dy.dtype)
        if need_dx:
            dx = dx.view(ctx.xshape)
        if need_dw:
            mg = getattr(weight, "main_grad", None)
            odt = torch.float32 if mg is not None else weight.dtype
            if wgrad:
                xc8, xcs = ctx.saved_tensors[1:]
                dw = mx_gemm(dyc[0], dyc[1], xc8, xcs, bwd, fwd, None, odt)
            else:  # M % 128 != 0: the saved operand is x itself
                dw = (dy2.t().float() @ ctx.saved_tensors[1].float()).to(odt)
            if mg is not None:
                from ..ops.fused import main_grad_placeholder

                mg.add_(dw)
                dw = main_grad_placeholder(weight)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            if _ext.use_native(dy2):
                db = _C().colsum(dy2, ctx.bias_dtype)
            else:
                db = dy2.float().sum(0).to(ctx.bias_dtype)
        return dx, dw, db, None, None


def mx_linear(x, weight, bias=None, fwd_format="e4m3", bwd_format="e5m2"):
    """y = x W^T (+ bias) with all three GEMMs on the MX kernel.
      forward  y  = x_row . W_row^T (+ bias)   x [.., K], W [N, K] in ``fwd_format``; x is quantised
               rowwise and colwise by one launch
      dgrad    dx = dy_row . (W_col)^T         dy in ``bwd_format``; W_col = codes [K, N], blocks along N
      wgrad    dW = dy_col . (x_col)^T         dy_col [N, M], x_col [K, M]: blocks along the tokens;
               fp32 and added into ``weight.main_grad`` when the parameter carries one, else the
               weight's dtype
      db       column sum of dy
    Saved for backward: x_col's codes and scales plus the weight (whose colwise codes the backward
    makes), not x. A forward shape ``mx_supported`` declines (K % 128, N % 8, a dtype other than
    bf16 / fp16 / fp32) runs ``torch.nn.functional.linear``; a backward GEMM whose own contraction
    the kernel declines (N % 128 for dx, tokens % 128 for dW) runs as a torch matmul."""
    fwd, bwd = _fmt(fwd_format), _fmt(bwd_format)
    K = x.shape[-1]
    M = x.numel() // max(K, 1)
    if (weight.dim() != 2 or weight.shape[1] != K or not mx_supported(M, K, weight.shape[0], _ext.use_native(x))
            or x.dtype not in _IN_DTYPES or weight.dtype not in _IN_DTYPES or weight.device != x.device):
        return torch.nn.functional.linear(x, weight, bias)
    return _MXLinearFn.apply(x, weight, bias, fwd, bwd)


class MXLinear(torch.nn.Linear):
    """``torch.nn.Linear`` whose forward is ``mx_linear``."""

    def __init__(self, in_features, out_features, bias=True, fwd_format="e4m3", bwd_format="e5m2", device=None,
                 dtype=None):
        super().__init__(in_features, out_features, bias=bias, device=device, dtype=dtype)
        self.fwd_format, self.bwd_format = fwd_format, bwd_format

    def forward(self, x):
        return mx_linear(x, self.weight, self.bias, self.fwd_format, self.bwd_format)
