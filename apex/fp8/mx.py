"""MXFP8 / MXFP4: OCP Microscaling fp8 and fp4 on gfx950's block-scaled MFMA, with the block scales in use.

Every 32 consecutive values along the contraction carry their own power-of-two scale (one E8M0
byte, 2^(s - 127)), computed from that block's own amax when it is quantised: no amax history, no
per-tensor state to checkpoint or all-reduce, and an outlier costs precision in its own block only.

  mx_quantize    x [R, C] -> (codes, scales) rowwise (blocks along C) and / or colwise (codes [C, R],
                 blocks along R), one launch (csrc/mx.hip)
  mx_gemm        C = (A . 2^(sa - 127)) (B . 2^(sb - 127))^T (+ bias), csrc/gemm_mx.hip; with an e2m1 b
                 (and an e2m1 or fp8 a) csrc/gemm_mx4.hip
  mx_dequantize  the values a (codes, scales) pair encodes — torch, for debugging and fallbacks
  mx_supported   the shape predicate of mx_gemm; callers use it to decline, not to crash
  mx_linear      autograd linear layer whose three GEMMs run on mx_gemm; ``MXLinear`` wraps it

Scale byte of a block: ``s = max(E - emax, 0)`` with E the biased fp32 exponent of the block's amax
and emax = 8 (e4m3) / 15 (e5m2) / 2 (e2m1); codes = sat(x * 2^(127 - s)) rounded to nearest even. A block that
holds an inf or a NaN gets ``s = 0xFF`` (the E8M0 NaN) and is converted unscaled the way the
per-tensor quantisers convert non-finite values (+-inf -> +-max, NaN -> -max).

``E2M1`` (MXFP4) has the grid +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}. Its codes are packed two to a byte along
the block direction, element 2 i in the low nibble of byte i and 2 i + 1 in the high nibble (the
``float4_e2m1fn_x2`` order): rowwise codes are [R, C / 2], colwise [C, R / 2]; scales as for fp8.

CPU tensors and ``APEX_FORCE_REFERENCE=1`` take a torch path with the same contract.
Nothing in ``Fp8Recipe`` / ``fp8_autocast`` routes to these functions: they are called directly.
"""
from __future__ import annotations

import torch

from .. import _ext
from . import E4M3, E5M2, FMT_MAX, _aligned, _C

__all__ = ["mx_quantize", "mx_dequantize", "mx_gemm", "mx_supported", "mx_linear", "MXLinear", "E2M1"]

E2M1 = 2
_MX_FMT_NAMES = {"e4m3": E4M3, "e5m2": E5M2, "e2m1": E2M1}  # (Fp8Recipe's own table has no e2m1)
_EMAX = {E4M3: 8, E5M2: 15, E2M1: 2}
_MAX = {**FMT_MAX, E2M1: 6.0}
_F8T = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}
_E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
_IN_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _fmt(f):
    f = _MX_FMT_NAMES.get(f, f) if isinstance(f, str) else f
    if f not in (E4M3, E5M2, E2M1):
        raise ValueError(f"mx: format {f!r}: expected E4M3 / E5M2 / E2M1 (or 'e4m3' / 'e5m2' / 'e2m1')")
    return f


def _e2m1_encode(p):
    """fp32 values in [-6, 6] -> e2m1 codes (int64), round to nearest, ties to the even code."""
    a = p.abs()
    # step 0.5 below 2, 1 below 4, 2 above: torch.round rounds halves to even, which is the even code
    # in each range (the codes' low bit alternates with the grid points of a range)
    n = torch.where(a < 2, torch.round(a * 2), torch.where(a < 4, torch.round(a) + 2, torch.round(a / 2) + 4))
    return n.to(torch.int64) | (torch.signbit(p).to(torch.int64) << 3)


def _e2m1_values(codes, dtype):
    """packed codes [R, K / 2] -> values [R, K]"""
    lut = torch.tensor(_E2M1_VALUES + tuple(-v for v in _E2M1_VALUES), dtype=dtype, device=codes.device)
    c = codes.to(torch.int64)
    return lut[torch.stack((c & 15, c >> 4), dim=-1).reshape(codes.shape[0], -1)]


def _ref_quantize_rows(x, fmt):
    """The contract in fp32 torch arithmetic: x [R, C] -> codes [R, C], scales [R, C / 32]."""
    R, C = x.shape
    xb = x.float().reshape(R, C // 32, 32)
    E = (xb.contiguous().view(torch.int32) & 0x7FFFFFFF).amax(dim=-1) >> 23
    bad = E == 255
    s = torch.where(bad, torch.full_like(E, 255), (E - _EMAX[fmt]).clamp(min=0))
    mult = torch.ldexp(torch.ones_like(s, dtype=torch.float32), torch.where(bad, torch.zeros_like(s), 127 - s))
    p = xb * mult.unsqueeze(-1)  # exact: a power of two
    p = torch.where(torch.isnan(p), torch.full_like(p, -_MAX[fmt]), p).clamp(-_MAX[fmt], _MAX[fmt])
    if fmt == E2M1:
        c = _e2m1_encode(p).reshape(R, C // 2, 2)
        return (c[..., 0] | (c[..., 1] << 4)).to(torch.uint8), s.to(torch.uint8)
    return p.to(_F8T[fmt]).view(torch.uint8).reshape(R, C), s.to(torch.uint8)


def mx_quantize(x, fmt=E4M3, rowwise=True, colwise=False):
    """x [R, C] (bf16 / fp16 / fp32) -> MX operands, one ``(codes, scales)`` pair per requested
    orientation (the pair itself when one is requested, ``(rowwise pair, colwise pair)`` for both),
    all from one launch that reads x once.
      rowwise  codes [R, C], scales [R, C / 32]; needs C % 32 == 0
      colwise  codes [C, R], scales [C, R / 32] (the transposed codes, blocks along R); R % 32 == 0
    ``E2M1`` codes are packed two to a byte, the even element in the low nibble: [R, C / 2], [C, R / 2].
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
    """(codes [R, K] — e2m1: packed [R, K / 2] —, scales [R, K / 32]) -> the encoded values in ``dtype``
    (a 0xFF scale: NaN)."""
    fmt = _fmt(fmt)
    s = scales.to(torch.int32)
    f = torch.ldexp(torch.ones_like(s, dtype=torch.float32), s - 127)
    f = torch.where(s == 255, torch.full_like(f, float("nan")), f)
    v = _e2m1_values(codes, torch.float32) if fmt == E2M1 else codes.view(_F8T[fmt]).to(torch.float32)
    return (v * f.repeat_interleave(32, dim=1)).to(dtype)


def mx_supported(M, K, N, native=True, fmt_a=E4M3, fmt_b=E4M3):
    """Can ``mx_gemm`` take a [M, K] x [N, K]^T product of these formats? The kernels (``native``, device
    tensors) need N % 8 == 0 and K % 128 == 0 — K % 256 == 0 for e2m1 x e2m1, whose K-tile is 256 and
    which takes no half tile — (their operands must also be contiguous and 16-byte aligned, which
    ``mx_quantize`` outputs are); the torch reference path only whole blocks, K % 32 == 0. An e2m1 ``a``
    against an fp8 ``b`` is supported by neither."""
    fmt_a, fmt_b = _fmt(fmt_a), _fmt(fmt_b)
    if fmt_a == E2M1 and fmt_b != E2M1:
        return False
    if not native:
        return M >= 1 and N >= 1 and K >= 32 and K % 32 == 0
    kt = 256 if fmt_a == E2M1 else 128
    return M >= 1 and K >= kt and K % kt == 0 and N >= 8 and N % 8 == 0 and max(M, N, K) < 2 ** 31 - 256


def mx_gemm(a, a_scales, b, b_scales, fmt_a=E4M3, fmt_b=E4M3, bias=None, out_dtype=torch.bfloat16):
    """C [M, N] = (a . 2^(a_scales - 127)) (b . 2^(b_scales - 127))^T (+ bias) in ``out_dtype`` (bf16 /
    fp16 / fp32) from an fp32 accumulator. a [M, K], b [N, K]: uint8 codes in ``fmt_a`` / ``fmt_b``;
    scales [M, K / 32], [N, K / 32]: E8M0 bytes; K % 128 == 0, N % 8 == 0 (``mx_supported``), all
    contiguous and 16-byte aligned. There is no alpha: MX has no per-tensor factor. An ``E2M1``
    operand is packed, [rows, K / 2]; b may be e2m1 with a in any format (K % 256 == 0 when both are),
    an e2m1 a needs an e2m1 b (``ValueError`` otherwise).

    A 0xFF scale byte (what ``mx_quantize`` gives a block with an inf or a NaN) is the E8M0 NaN, and
    the MFMA honours it (measured on MI355X, pinned by tests/test_mx_gpu.py::test_nan_scale): every
    output element whose row of a or of b has such a block is NaN, whatever that block's codes —
    all-zero codes included — and no other element is touched; e2m1 operands behave the same
    (tests/test_mx4_gpu.py::test_nan_scale). The torch path does the same."""
    fmt_a, fmt_b = _fmt(fmt_a), _fmt(fmt_b)
    if fmt_a == E2M1 and fmt_b != E2M1:
        raise ValueError("mx_gemm: an e2m1 a needs an e2m1 b (fp4 x fp8 is not built; fp8 x fp4 is)")
    pa, pb = (2 if f == E2M1 else 1 for f in (fmt_a, fmt_b))   # codes per byte
    M, K = a.shape[0], a.shape[1] * pa
    N = b.shape[0]
    if not mx_supported(M, K, N, _ext.use_native(a), fmt_a, fmt_b) or tuple(b.shape) != (N, K // pb) or \
            tuple(a_scales.shape) != (M, K // 32) or tuple(b_scales.shape) != (N, K // 32):
        raise ValueError(f"mx_gemm: unsupported shapes a {tuple(a.shape)} / {tuple(a_scales.shape)}, "
                         f"b {tuple(b.shape)} / {tuple(b_scales.shape)} (K % 128 == 0, e2m1 x e2m1 K % 256 == 0, "
                         f"N % 8 == 0, e2m1 codes [rows, K / 2])")
    if bias is not None and bias.dtype != out_dtype:
        bias = bias.to(out_dtype)
    if _ext.use_native(a):
        bias = None if bias is None else _aligned(bias.detach())
        if fmt_b == E2M1:
            return _C().gemm_mx4(_aligned(a), _aligned(a_scales), _aligned(b), _aligned(b_scales), fmt_a, bias, out_dtype)
        return _C().gemm_mx(_aligned(a), _aligned(a_scales), _aligned(b), _aligned(b_scales), fmt_a, fmt_b, bias, out_dtype)

    def val(codes, scales, fmt):  # float64 (0xFF: NaN, also times a zero code)
        s = scales.to(torch.int32)
        f = torch.ldexp(torch.ones(s.shape, dtype=torch.float64, device=s.device), s - 127)
        f = torch.where(s == 255, torch.full_like(f, float("nan")), f)
        v = _e2m1_values(codes, torch.float64) if fmt == E2M1 else codes.view(_F8T[fmt]).to(torch.float64)
        return v * f.repeat_interleave(32, dim=1)

    c = (val(a, a_scales, fmt_a) @ val(b, b_scales, fmt_b).t()).float()
    if bias is not None:
        c = c + bias.float()
    return c.to(out_dtype)


class _MXLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, fwd, bwd, wfmt):
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        M, N = x2.shape[0], weight.shape[0]
        # dW [N, K] = dy_col [N, M] . x_col [K, M]^T contracts over the M tokens: x's colwise codes are
        # made by the same launch as the forward operand and are what is kept for it
        wgrad = ctx.needs_input_grad[1] and mx_supported(N, M, K, _ext.use_native(x), bwd, fwd)
        if wgrad:
            (x8, xs), xcol = mx_quantize(x2, fwd, True, True)
        else:
            (x8, xs), xcol = mx_quantize(x2, fwd, True, False), None
        w8, ws = mx_quantize(weight, wfmt, True, False)
        y = mx_gemm(x8, xs, w8, ws, fwd, wfmt, bias, x.dtype)
        ctx.wfmt = wfmt
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
        dgrad = need_dx and mx_supported(M, N, K, _ext.use_native(dy), bwd, ctx.wfmt)
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
            wc8, wcs = mx_quantize(weight, ctx.wfmt, False, True)  # codes [K, N], blocks along N
            dx = mx_gemm(dyr[0], dyr[1], wc8, wcs, bwd, ctx.wfmt, None, dy.dtype)
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
        return dx, dw, db, None, None, None


def mx_linear(x, weight, bias=None, fwd_format="e4m3", bwd_format="e5m2", weight_format=None):
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
    the kernel declines (N % 128 for dx, tokens % 128 for dW) runs as a torch matmul.

    ``weight_format`` (None: ``fwd_format``) is the format of W in the forward and dgrad GEMMs:
    ``"e2m1"`` runs them as fp8 x fp4 (x, dy in fp8 against MXFP4 weights), wgrad unchanged.
    ``fwd_format="e2m1"`` makes x fp4 too: the forward is fp4 x fp4 (K % 256 == 0), the kept x_col is
    fp4 and wgrad is dy_col (fp8) x x_col (fp4); the weight is then e2m1 as well (an fp4 x against an
    fp8 weight is not built). ``bwd_format="e2m1"`` raises ``ValueError``: fp4 gradients need
    stochastic rounding, which this layer does not have."""
    fwd, bwd = _fmt(fwd_format), _fmt(bwd_format)
    wfmt = fwd if weight_format is None else _fmt(weight_format)
    if bwd == E2M1:
        raise ValueError("mx_linear: bwd_format 'e2m1' is not supported (fp4 gradients need stochastic rounding)")
    if fwd == E2M1 and wfmt != E2M1:
        raise ValueError("mx_linear: fwd_format 'e2m1' needs an e2m1 weight_format")
    K = x.shape[-1]
    M = x.numel() // max(K, 1)
    if (weight.dim() != 2 or weight.shape[1] != K
            or not mx_supported(M, K, weight.shape[0], _ext.use_native(x), fwd, wfmt)
            or x.dtype not in _IN_DTYPES or weight.dtype not in _IN_DTYPES or weight.device != x.device):
        return torch.nn.functional.linear(x, weight, bias)
    return _MXLinearFn.apply(x, weight, bias, fwd, bwd, wfmt)


class MXLinear(torch.nn.Linear):
    """``torch.nn.Linear`` whose forward is ``mx_linear``."""

    def __init__(self, in_features, out_features, bias=True, fwd_format="e4m3", bwd_format="e5m2", device=None,
                 dtype=None, weight_format=None):
        super().__init__(in_features, out_features, bias=bias, device=device, dtype=dtype)
        self.fwd_format, self.bwd_format, self.weight_format = fwd_format, bwd_format, weight_format

    def forward(self, x):
        return mx_linear(x, self.weight, self.bias, self.fwd_format, self.bwd_format, self.weight_format)
