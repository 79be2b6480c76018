"""Float64 reference of the MXFP4 path (csrc/mx.hip format 2, csrc/gemm_mx4.hip), beside mx_reference: a plain helper.
e2m1 code = sign << 3 | index into VALUES; packed: element 2 i in the low nibble of byte i, 2 i + 1 in the high.
Quantiser, to the bit: per 1 x 32 block E = biased fp32 exponent of amax, s = max(E - 2, 0), codes = nearest grid
point of sat(x * 2**(127 - s)), a tie to the even code, a zero keeps its sign; a block with an inf or a NaN: s = 0xFF,
multiplier 1, +-inf -> +-6, NaN -> 0xF. GEMM bound: mx_reference.expected (the instruction is MXFP8's)."""
import torch

import mx_reference as X

E2M1 = 2
VALUES = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
MIDS = (VALUES[:-1] + VALUES[1:]) / 2
TIE_UP = torch.arange(7) % 2 == 1            # the midpoint above code i goes up when code i + 1 is even
expected = X.expected


def pack(codes):
    c = codes.to(torch.int64)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8)


def decode(packed):
    """packed codes [R, K / 2] -> float64 values [R, K]"""
    p = packed.to(torch.int64)
    c = torch.stack((p & 15, p >> 4), dim=-1).reshape(packed.shape[0], -1)
    return torch.where((c & 8) != 0, -VALUES[c & 7], VALUES[c & 7])


def quantize_ref(x):
    """x [R, C] -> (packed codes [R, C / 2], scales [R, C / 32]) rowwise; colwise is quantize_ref(x.t())."""
    R, C = x.shape
    xb = x.double().reshape(R, C // 32, 32)
    a = xb.abs()
    bad = ~torch.isfinite(a).all(dim=-1)
    amax = torch.where(torch.isnan(a), torch.zeros_like(a), a).amax(dim=-1)
    _, ex = torch.frexp(amax)
    E = torch.where(amax >= 2.0 ** -126, ex - 1 + 127, torch.zeros_like(ex)).to(torch.int64)
    s = torch.where(bad, torch.full_like(E, 255), (E - 2).clamp(0, 254))
    p = xb * torch.where(bad, torch.ones_like(amax), torch.exp2((127 - s).double())).unsqueeze(-1)
    m = p.abs().unsqueeze(-1)                 # (above 6: past every midpoint, code 7)
    codes = ((m > MIDS) | ((m == MIDS) & TIE_UP)).sum(-1) | (torch.signbit(p).to(torch.int64) << 3)
    codes = torch.where(torch.isnan(p), torch.full_like(codes, 0xF), codes)
    return pack(codes.reshape(R, C)), s.to(torch.uint8)


def scaled(packed, scales):
    """The float64 values of an MXFP4 operand: decode(codes) * 2**(scales - 127) per 32-block."""
    return decode(packed) * torch.exp2(scales.double() - 127.0).repeat_interleave(32, dim=1)


def operand(t, fmt, quantised=True):
    """Float64 values of t [R, C] quantised rowwise in fmt (E2M1 or an fp8 format), or t itself."""
    if not quantised:
        return t.double()
    return scaled(*quantize_ref(t)) if fmt == E2M1 else X.scaled(*X.quantize_ref(t, fmt), fmt)


def linear_expected(x, w, bias, dy, fwd, bwd, wfmt, supported):
    """mx_reference.linear_expected with a weight format: each GEMM from the quantised operands it consumes where
    supported(M', K', N', fmt_a=, fmt_b=) accepts it, the plain ones where the layer runs it unquantised."""
    (M, K), N = x.shape, w.shape[0]
    fw, dg, wg = supported(M, K, N, fmt_a=fwd, fmt_b=wfmt), supported(M, N, K, fmt_a=bwd, fmt_b=wfmt), \
        supported(N, M, K, fmt_a=bwd, fmt_b=fwd)
    return {"y": expected(operand(x, fwd, fw), operand(w, wfmt, fw), K, x.dtype, bias),
            "dx": expected(operand(dy, bwd, dg), operand(w.t(), wfmt, dg), N, x.dtype),
            "dw": expected(operand(dy.t(), bwd, wg), operand(x.t(), fwd, wg), M, torch.float32),
            "db": tuple(t.reshape(-1) for t in expected(dy.double().t(), torch.ones(1, M, dtype=torch.float64), M, bias.dtype))}
