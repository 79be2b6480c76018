"""Reference of the MXFP8 path (csrc/mx.hip, csrc/gemm_mx.hip, apex/fp8/mx.py), in float64, on top of
fp8_reference's OCP codec. A plain helper module: no tests, it never calls the extension.

Quantiser, to the bit: per 1 x 32 block, amax = max |x| (NaN dropped), E = biased fp32 exponent of amax (0 for
zero and fp32 subnormals), s = clamp(E - emax, 0, 254), codes = encode(sat(x * 2**(127 - s))). A block holding an
inf or a NaN: s = 0xFF, codes of the unscaled values with fp8_reference's non-finite rule (NAN_CODE).

GEMM bound: fp8_reference's, acc_units(K) * 2**-24 * cond + HALF_ULP |ref| + TINY with cond = |A_scaled| |B_scaled|^T,
with ACC_MX in place of ACC_HW when the measurement with unequal block scales asks for it (see ACC_MX).
"""
import torch

from fp8_reference import ACC_HW, BK8, E24, HALF_ULP, NAN_CODE, TINY, decode, encode, sat  # noqa: F401

EMAX = {0: 8, 1: 15}
# Accumulator constant of the block-scaled instruction, by fp8_reference's rule for ACC_HW: the worst
# |err| / (2**-24 cond) over the dense cases of tests/test_mx_gpu.py against the float64 reference
# (profiles/mx_numerics_worst.txt), doubled and rounded up to a power of two — if that exceeds ACC_HW.
ACC_MX = ACC_HW


def acc_units(K):
    return ACC_MX + 2.0 * K / BK8


def quantize_ref(x, fmt):
    """x [R, C] -> (codes [R, C], scales [R, C / 32]) rowwise; colwise is quantize_ref(x.t(), fmt)."""
    R, C = x.shape
    xb = x.double().reshape(R, C // 32, 32)
    a = xb.abs()
    bad = ~torch.isfinite(a).all(dim=-1)
    amax = torch.where(torch.isnan(a), torch.zeros_like(a), a).amax(dim=-1)
    _, ex = torch.frexp(amax)                                  # amax = m * 2**ex, m in [0.5, 1)
    E = torch.where(amax >= 2.0 ** -126, ex - 1 + 127, torch.zeros_like(ex)).to(torch.int64)
    s = (E - EMAX[fmt]).clamp(0, 254)
    s = torch.where(bad, torch.full_like(s, 255), s)
    mult = torch.where(bad, torch.ones_like(amax), torch.pow(torch.tensor(2.0, dtype=torch.float64), (127 - s).double()))
    p = xb * mult.unsqueeze(-1)
    codes = encode(sat(p, fmt), fmt)
    codes = torch.where(torch.isnan(p), torch.full_like(codes, NAN_CODE[fmt]), codes)
    return codes.reshape(R, C), s.to(torch.uint8)


def scaled(codes, scales, fmt):
    """The float64 values of an MX operand: decode(codes) * 2**(scales - 127) per 32-block."""
    f = torch.pow(torch.tensor(2.0, dtype=torch.float64, device=codes.device), scales.double() - 127.0)
    return decode(codes, fmt) * f.repeat_interleave(32, dim=1)


def expected(a, b, K, odt, bias=None):
    """(ref, bound) of a b^T (+ bias) for float64 operand values a [M, K], b [N, K] rounded once to odt."""
    ref = a @ b.t()
    bound = acc_units(K) * E24 * (a.abs() @ b.abs().t())
    if bias is not None:
        ref = ref + bias.double()
    return ref, bound + HALF_ULP[odt] * ref.abs() + TINY[odt]


def linear_expected(x, w, bias, dy, fwd, bwd, supported):
    """{name: (ref, bound)} of mx_linear's y, dx, dW, db for x [M, K], w [N, K], dy [M, N]: each GEMM from the
    float64 values of the operands it consumes — the quantised ones where supported(M', K', N') accepts the GEMM
    (contraction K'), the plain ones where the layer runs that GEMM unquantised. dW's bound is for an fp32 output."""
    (M, K), N = x.shape, w.shape[0]

    def op(t, fmt, colwise, ok):
        return scaled(*quantize_ref(t.t() if colwise else t, fmt), fmt) if ok else (t.t() if colwise else t).double()

    fw, dg, wg = supported(M, K, N), supported(M, N, K), supported(N, M, K)
    out = {"y": expected(op(x, fwd, False, fw), op(w, fwd, False, fw), K, x.dtype, bias),
           "dx": expected(op(dy, bwd, False, dg), op(w, fwd, True, dg), N, x.dtype),
           "dw": expected(op(dy, bwd, True, wg), op(x, fwd, True, wg), M, torch.float32)}
    if bias is not None:
        out["db"] = expected(dy.double().t(), torch.ones(1, M, dtype=torch.float64), M, bias.dtype)
        out["db"] = tuple(t.reshape(-1) for t in out["db"])
    return out
