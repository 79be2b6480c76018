"""Reference of the fp8 path (csrc/fp8.hip, csrc/fp8_pack.h, the uint8 instantiations of the MFMA GEMM,
gemm_tt_f8 and the Q8 side outputs of the GEMM epilogue): an OCP fp8 codec written from the specification,
the quantisers and the delayed-scaling update to the bit, the float64 fp8 GEMM with its per-element bound,
CPU emulations with mutants, and the shared case tables.

A plain helper module like gemm_reference.py: no tests, no fixtures, it never calls the extension and it never
touches torch.float8_*. tests/test_fp8_reference.py (the codec against torch's CPU casts, emulations and
mutants, on the CPU) and tests/test_fp8_numerics_gpu.py (the HIP kernels) share everything below.

Codec (OCP 8-bit floating point specification, v1.0). A code is sign | exponent | mantissa.
  e4m3fn  4 exponent bits, bias 7, 3 mantissa bits; no infinity, NaN = S.1111.111 (0x7f / 0xff), so the
          largest finite value is S.1111.110 = 1.75 * 2**8 = 448; subnormals m * 2**-9.
  e5m2    5 exponent bits, bias 15, 2 mantissa bits, IEEE-like: S.11111.00 = inf, S.11111.mm = NaN, largest
          finite 1.75 * 2**15 = 57344; subnormals m * 2**-16.
encode() rounds to nearest, ties to even, in exact float64 arithmetic (scaling by a power of two and
torch.round, which rounds halves to even); the quantisers saturate first, as the kernels do.

Quantisers, to the bit:  q = encode(sat(fl32(fl32(x) * s))). The product of two fp32 values is exact in
float64, so fl32 of the float64 product is the correctly rounded fp32 product. amax = max |x| exactly (NaN
elements dropped: every amax of the kernels is an fmaxf / v_max3_f32 chain). Current scaling:
s = fl32(smax / a), scale_inv = fl32(1 / s) (a float64 quotient of two fp32 values rounded to fp32 is the
correctly rounded fp32 quotient: 53 >= 2 * 24 + 2), s = 1 for a = 0 or a non-finite a.
update_scales follows the header comment of fp8.hip in the kernel's fp32 operation order:
hist[idx] = amax_cur if finite else 0; a = max(hist); if a > 0: scale = fl32(fl32(fmt_max / a) * margin),
scale_inv = fl32(1 / scale), else both stay; amax_cur = 0.

Non-finite elements (measured once on gfx950 and pinned by the GPU test; stated in fp8.hip's header):
+-inf saturates to +-max and makes amax inf; NaN is dropped by every amax and its code is NAN_CODE[fmt].

fp8 GEMM. Every e4m3 / e5m2 value is exact in float64 (and in bf16 and fp16). alpha = fl32(alpha_a * alpha_b),
acc* = alpha * A B^T (NT) or alpha * A^T B (weight-gradient form), cond = |alpha| |A| |B|^T. The epilogues,
E_act / E_g, the bias-gradient and the slab-combine terms are gemm_reference's. Differences from the 16-bit
bound:
  accumulator   delta = (ACC_HW + 2 K / 128) * 2**-24 * cond. The derived term of the 16-bit file, K * 2**-23 *
                cond (exact products, K - 1 additions each within one ulp of a partial sum, in any order), does
                not hold for v_mfma_scale_f32_16x16x128_f8f6f4: its internal summation over the 128 exact
                products of one instruction is undocumented, and on an MI355X the dense cases at K = 128 exceeded
                the derived term (error / bound up to 1.39) while every integer case stayed bit-exact. The
                error does not grow with K (the ratio fell from 1.2 at K = 128 to 0.7 at K = 384 under the
                K-proportional term): it is an error of each instruction relative to its own 128 products, and
                those conds add up to cond. ACC_HW is therefore MEASURED: the worst |err| / (2**-24 cond) over
                the dense tables of tests/test_fp8_numerics_gpu.py (the `none` epilogue of every NT shape and
                the fp32 output of every weight-gradient case; profiles/fp8_numerics_worst.txt has the figure),
                doubled and rounded up to a power of two. The K / 128 - 1 fp32 additions of instruction results
                into the accumulator stay derived: 2**-23 cond each. No other term was fitted.
  staged value  rnd_T(fl32(acc * alpha)): one fp32 rounding more than the 16-bit path, 2**-24 |acc*|
                (gemm_reference.expected's `stage` argument).
  weight grad   the slab is fl32(acc_s * alpha): 2**-24 |slab_s| more per slab.
Q8 side outputs: codes = encode(sat(fl32(C_stored * q8_scale))) and amax = max |C_stored|, both exact once
the stored C is known.
Nothing here was fitted to a GPU run except NAN_CODE, which is a measurement by design.
"""
from __future__ import annotations

import functools
import math

import torch

import gemm_reference as R
from mt_reference import BF16, DT_NAME, F16, F32, HALF_ULP, TINY, f32  # noqa: F401

E4M3, E5M2 = 0, 1
FMTS = [E4M3, E5M2]
FMT_NAME = {E4M3: "e4m3", E5M2: "e5m2"}
MBITS = {E4M3: 3, E5M2: 2}
BIAS = {E4M3: 7, E5M2: 15}
FMT_MAX = {E4M3: 448.0, E5M2: 57344.0}
MAX_CODE = {E4M3: 0x7e, E5M2: 0x7b}
SCALES = [1.0, 37.5, 2.0 ** -7, 1e4, 3e38]
IN_DTYPES = [BF16, F16, F32]
E23, E24 = R.E23, R.E24
BK8 = 128            # the fp8 kernels' K-tile
# accumulator term (ACC_HW + 2 K / 128) * 2**-24 * cond. ACC_HW is measured, not derived: the worst
# |err| / (2**-24 cond) seen on an MI355X over the dense NT (`none` epilogue) and weight-gradient (fp32 output)
# tables of tests/test_fp8_numerics_gpu.py was 355.3 (profiles/fp8_numerics_worst.txt); twice that, rounded up to a
# power of two (module docstring)
ACC_HW = 1024.0
# the code a NaN element becomes: v_med3_f32(NaN, -max, max) returns min3 of its operands when one is a
# NaN, and min ignores a NaN operand, so NaN saturates to -max (measured on gfx950, pinned by
# test_fp8_numerics_gpu.py::test_nonfinite_elements)
NAN_CODE = {E4M3: 0xfe, E5M2: 0xfb}


# ----------------------------------------------------------------------------
# codec
# ----------------------------------------------------------------------------
def decode(codes, fmt):
    """uint8 codes -> float64 values (on codes' device)."""
    c = codes.to(torch.int64)
    mb, bias = MBITS[fmt], BIAS[fmt]
    sign = torch.where((c & 0x80) != 0, -1.0, 1.0).double()
    e = (c & 0x7f) >> mb
    m = (c & ((1 << mb) - 1)).double()
    sub = m * 2.0 ** (1 - bias - mb)
    nor = (1.0 + m / (1 << mb)) * torch.pow(torch.tensor(2.0, dtype=torch.float64, device=c.device), (e - bias).double())
    v = torch.where(e == 0, sub, nor)
    if fmt == E4M3:
        v = torch.where((c & 0x7f) == 0x7f, torch.full_like(v, float("nan")), v)
    else:
        top = e == 31
        v = torch.where(top & (m == 0), torch.full_like(v, float("inf")), v)
        v = torch.where(top & (m != 0), torch.full_like(v, float("nan")), v)
    return sign * v


def encode(x, fmt, rounding="rne", saturate=True, bias=None, flush_subnormals=False):
    """Values (any float dtype, taken exactly as float64) -> uint8 codes. Round to nearest even; a magnitude
    that rounds above the format's maximum becomes the maximum (saturate) or the format's overflow code
    (e4m3: NaN, e5m2: inf). NaN -> 0x7f | sign. The keyword arguments exist for the mutants of
    tests/test_fp8_reference.py: rounding "trunc" / "away", another exponent bias (fnuz: 8), flushed subnormals."""
    x = x.double()
    mb = MBITS[fmt]
    bias = BIAS[fmt] if bias is None else bias
    emin = 1 - bias
    emax = (15 if fmt == E4M3 else 30) - bias
    fmax = (2.0 - 2.0 ** -mb if fmt == E5M2 else 1.75) * 2.0 ** emax
    neg = torch.signbit(x)
    a = x.abs()
    nan = torch.isnan(a)
    a = torch.where(nan, torch.zeros_like(a), a)
    if saturate:
        a = a.clamp(max=fmax)
    _, ex = torch.frexp(a)                                   # a = m * 2**ex, m in [0.5, 1)
    e = (ex - 1).clamp(min=emin, max=emax + 1).to(torch.int64)
    q = torch.pow(torch.tensor(2.0, dtype=torch.float64, device=x.device), (e - mb).double())
    n = a / q                                                # exact: a power-of-two scaling
    n = torch.where(torch.isinf(a), torch.full_like(n, 2.0 ** (mb + 2)), n).clamp(max=2.0 ** (mb + 2))
    if rounding == "rne":
        r = torch.round(n)
    elif rounding == "trunc":
        r = torch.floor(n)
    else:
        r = torch.floor(n + 0.5)
    r = r.to(torch.int64)
    carry = r >= (2 << mb)
    e = torch.where(carry, e + 1, e)
    r = torch.where(carry, torch.full_like(r, 1 << mb), r)
    subn = r < (1 << mb)                                     # (only at e == emin)
    code = torch.where(subn, r, ((e + bias) << mb) | (r - (1 << mb)))
    if flush_subnormals:
        code = torch.where(subn, torch.zeros_like(code), code)
    over = (e > emax) | torch.isinf(a) | ((fmt == E4M3) & (e == emax) & (r == (2 << mb) - 1))
    if fmt == E4M3:
        over_code = 0x7e if saturate else 0x7f
    else:
        over_code = 0x7b if saturate else 0x7c
    code = torch.where(over, torch.full_like(code, over_code), code)
    code = torch.where(nan, torch.full_like(code, 0x7f), code)
    return (code | (neg.to(torch.int64) << 7)).to(torch.uint8)


def sat(x, fmt):
    """Clamp to the format's finite range; NaN stays NaN."""
    return x.clamp(-FMT_MAX[fmt], FMT_MAX[fmt])


# ----------------------------------------------------------------------------
# quantisers, to the bit
# ----------------------------------------------------------------------------
def scaled(x, s):
    """fl32(fl32(x) * s) for an fp32 scale s: the float64 product (exact) rounded once to fp32."""
    return (x.double() * float(f32(s))).float()


def quantize_ref(x, s, fmt, nan_code=True):
    """Codes of the quantisers: encode(sat(fl32(x * s))); a NaN element becomes NAN_CODE[fmt]."""
    p = scaled(x, s)
    codes = encode(sat(p, fmt), fmt)
    if nan_code:
        codes = torch.where(torch.isnan(p), torch.full_like(codes, NAN_CODE[fmt]), codes)
    return codes


def amax_ref(x, prev=0.0):
    """max(prev, max |x|) as the kernels take it: exact, NaN elements dropped, inf kept."""
    a = x.double().abs()
    a = torch.where(torch.isnan(a), torch.zeros_like(a), a)
    return max(float(prev), float(a.max()) if a.numel() else 0.0)


def current_scale(a, smax):
    """(s, scale_inv) of current scaling from the measured amax a: fp32 values as Python floats."""
    a = f32(a) if math.isfinite(a) else a
    s = f32(f32(smax) / a) if (a > 0.0 and math.isfinite(a)) else 1.0
    return s, f32(1.0 / s)


def update_scales_ref(hist, amax_cur, scale, scale_inv, fmt_max, n_slots, idx, margin_scale):
    """The state after one fp8_update_scales call (fp32 CPU tensors in, new tensors out; slots >= n_slots
    untouched). fp32 operations in the kernel's order: torch's fp32 CPU division and product are IEEE."""
    hist, amax_cur, scale, scale_inv = (t.clone() for t in (hist, amax_cur, scale, scale_inv))
    n = n_slots
    cur = amax_cur[:n]
    hist[:n, idx] = torch.where(torch.isfinite(cur), cur, torch.zeros_like(cur))
    a = hist[:n].max(dim=1).values
    ok = (a > 0) & torch.isfinite(a)
    sc = (fmt_max[:n] / a) * torch.tensor(margin_scale, dtype=torch.float32)
    scale[:n] = torch.where(ok, sc, scale[:n])
    scale_inv[:n] = torch.where(ok, 1.0 / sc, scale_inv[:n])
    amax_cur[:n] = 0.0
    return hist, amax_cur, scale, scale_inv


# ---- emulations in the kernels' structure, with the mutants of the CPU test -----------------------------
Q_MUTANTS = ["trunc", "ties_away", "no_saturation", "fnuz", "flush_subnormals", "amax_after_scale",
             "amax_misses_tail", "scale_inv_is_s"]
QT_MUTANTS = ["tile_rc_swapped"]
US_MUTANTS = ["hist_max_short", "margin_inverted", "nonfinite_poisons"]


def _emu_encode(p, fmt, mut):
    kw = {}
    if mut == "trunc":
        kw["rounding"] = "trunc"
    elif mut == "ties_away":
        kw["rounding"] = "away"
    elif mut == "fnuz" and fmt == E4M3:
        kw["bias"] = 8
    elif mut == "flush_subnormals":
        kw["flush_subnormals"] = True
    if mut == "no_saturation":
        return encode(p, fmt, saturate=False)
    return encode(sat(p, fmt), fmt, **kw)


def emu_quantize(x, s, fmt, cur=None, smax=None, mut=None):
    """fp8_quantize in fp32 torch arithmetic, vector body and scalar tail apart -> (codes, amax, s, scale_inv)."""
    sinv = None
    if cur is not None:
        a = torch.tensor(cur, dtype=torch.float32)
        ok = bool(a > 0) and bool(torch.isfinite(a))
        s32 = torch.tensor(smax, dtype=torch.float32) / a if ok else torch.tensor(1.0)
        sinv = float(s32 if mut == "scale_inv_is_s" else 1.0 / s32)
    else:
        s32 = torch.tensor(s, dtype=torch.float32)
    n = x.numel()
    nv = n // 8 * 8
    xf = x.reshape(-1).float()
    parts, mx = [], 0.0
    for lo, hi in ((0, nv), (nv, n)):
        v = xf[lo:hi]
        p = v * s32
        if hi > lo and not (mut == "amax_misses_tail" and lo == nv):
            mx = amax_ref(p if mut == "amax_after_scale" else v, mx)
        parts.append(_emu_encode(p, fmt, mut))
    return torch.cat(parts).view(x.shape), mx, float(s32), sinv


def emu_quantize_t(x, s, fmt, mut=None):
    """fp8_quantize_t tile by tile: y[c][r] = quant(x[r][c]) over 64 x 64 tiles -> (codes [C, R], amax)."""
    Rr, Cc = x.shape
    s32 = torch.tensor(s, dtype=torch.float32)
    y = torch.zeros(Cc, Rr, dtype=torch.uint8)
    for r0 in range(0, Rr, 64):
        for c0 in range(0, Cc, 64):
            t = _emu_encode(x[r0:r0 + 64, c0:c0 + 64].float() * s32, fmt, None)
            if mut == "tile_rc_swapped" and t.shape == (64, 64):
                y[c0:c0 + 64, r0:r0 + 64] = t          # the tile lands where it belongs, untransposed
            else:
                y[c0:c0 + 64, r0:r0 + 64] = t.t()
    return y, amax_ref(x)


def emu_update_scales(hist, amax_cur, scale, scale_inv, fmt_max, n_slots, idx, margin_scale, mut=None):
    """update_scales_kernel one slot (thread) at a time, fp32 scalars."""
    hist, amax_cur, scale, scale_inv = (t.clone() for t in (hist, amax_cur, scale, scale_inv))
    L = hist.shape[1]
    m = torch.tensor(margin_scale, dtype=torch.float32)
    for sl in range(n_slots):
        cur = amax_cur[sl]
        hist[sl, idx] = cur if (bool(torch.isfinite(cur)) or mut == "nonfinite_poisons") else 0.0
        a = torch.tensor(0.0)
        for k in range(L - 1 if (mut == "hist_max_short" and L > 1) else L):
            a = torch.maximum(a, hist[sl, k]) if not bool(torch.isnan(hist[sl, k])) else a
        if bool(a > 0) and bool(torch.isfinite(a)):
            sc = fmt_max[sl] / a / m if mut == "margin_inverted" else fmt_max[sl] / a * m
            scale[sl] = sc
            scale_inv[sl] = 1.0 / sc
        elif mut == "nonfinite_poisons" and bool(torch.isinf(a)):
            scale[sl] = 0.0
            scale_inv[sl] = float("inf")
        amax_cur[sl] = 0.0
    return hist, amax_cur, scale, scale_inv


# ----------------------------------------------------------------------------
# tables of the quantiser tests
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bit_patterns(dtype, finite_only=True):
    """Every bf16 / fp16 bit pattern that is not a NaN (finite_only: nor an infinity), in pattern order."""
    assert dtype in (BF16, F16)
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    keep = torch.isfinite(x.float()) if finite_only else ~torch.isnan(x.float())
    return x[keep]


def _f32_neighbours(v):
    v = v.float()
    inf = torch.tensor(float("inf"))
    return torch.cat([v, torch.nextafter(v, inf), torch.nextafter(v, -inf)])


@functools.lru_cache(maxsize=None)
def boundary_set(fmt):
    """fp32 inputs on and around every rounding boundary of the format: every representable value, every
    midpoint between neighbours (half the smallest subnormal and the midpoint between the maximum and the
    next power step among them), the fp32 neighbours of each on both sides, +-max and its neighbours, +-0 —
    each also divided by every scale of SCALES (and the neighbours of the quotient), so that the scaled
    product lands on the boundaries too."""
    codes = torch.arange(0, MAX_CODE[fmt] + 1, dtype=torch.uint8)
    vals = decode(codes, fmt)                                       # 0 .. max, ascending
    step = vals[-1] - vals[-2]
    grid = torch.cat([vals, vals[-1:] + step])                      # (+ the value one step past the maximum)
    mids = (grid[:-1] + grid[1:]) / 2                               # exact in float64 and in fp32
    pos = torch.cat([grid, mids])
    pts = [_f32_neighbours(pos)]
    for s in SCALES:
        qv = (pos / float(f32(s))).float()
        pts.append(_f32_neighbours(qv[torch.isfinite(qv)]))
    p = torch.cat(pts)
    p = torch.cat([p, -p, torch.tensor([0.0, -0.0, 3.0e38, -3.0e38, 2.0 ** -149, -2.0 ** -126])])
    return p[torch.isfinite(p)].contiguous()


def quant_table(dtype, fmt):
    """The 1-D input table of a quantiser test: all finite patterns (16-bit), the boundary set (fp32). Built once
    and shared: callers leave it unchanged."""
    return boundary_set(fmt) if dtype == F32 else bit_patterns(dtype)


QUANT_LENGTHS = [3, 8 * 256 + 5, 2 ** 21 + 8 * 256 + 3]   # scalar tail alone; vector + tail; a second grid stride
QT_SHAPES = [(1, 1), (7, 9), (8, 64), (64, 8), (64, 64), (65, 63), (130, 72), (300, 200)]


def table_index(n, L):
    """n indices into a table of L entries: every entry when n >= L, at positions that move against the 8-wide
    vectors (an odd stride)."""
    return (torch.arange(n, dtype=torch.int64) * 7 + 3) % L


def amax_cases(dtype, lengths=tuple(QUANT_LENGTHS)):
    """(name, x) inputs of the amax tests, per length class: the largest magnitude a negative last element (the
    scalar tail), the largest in the vector body, negative values only, -0 alone."""
    out = []
    for n in lengths:
        g = R._gen(f"amax-{n}-{DT_NAME[dtype]}")
        x = torch.randn(n, generator=g).to(dtype)
        tail = x.clone()
        tail[-1] = -9.5
        body = x.clone()
        body[0] = 11.25
        out += [(f"n{n}-tail", tail), (f"n{n}-body", body), (f"n{n}-negative", -x.abs() - 0.125),
                (f"n{n}-minus-zero", torch.full((n,), -0.0, dtype=dtype))]
    return out


US_SLOTS, US_N = 300, 290            # buffers of 300 slots (a second block of 256), the last ten left alone
US_ZERO_SLOT = 7                     # a slot whose window stays all zero: its scale must stay
US_MARGINS = [1.0, 0.5, 2.0 ** -3]   # one per call


def update_scales_scenario(hist_len):
    """(state, calls): state = (hist, amax_cur, scale, scale_inv, fmt_max) before the first of three calls, calls
    = [(amax_cur to set before the call, idx, margin_scale)]. The index wraps (hist_len - 2, hist_len - 1, 0);
    the window of some slots holds its maximum in its last entry; inf and NaN amaxes arrive in every call."""
    g = R._gen(f"update-{hist_len}")
    hist = torch.rand(US_SLOTS, hist_len, generator=g) * 4.0
    hist[torch.arange(0, US_SLOTS, 3), hist_len - 1] = 5.0 + torch.rand(US_SLOTS // 3, generator=g)
    hist[US_ZERO_SLOT] = 0.0
    scale = torch.rand(US_SLOTS, generator=g) + 3.0
    scale_inv = torch.rand(US_SLOTS, generator=g) + 0.25
    fmt_max = torch.where(torch.arange(US_SLOTS) % 2 == 0, FMT_MAX[E4M3], FMT_MAX[E5M2]).float()
    calls = []
    for i, idx in enumerate((hist_len - 2 + i) % hist_len for i in range(3)):
        a = torch.rand(US_SLOTS, generator=g) * (10.0 ** (i - 1)) * 7.0
        a[5 + i::17] = float("inf")
        a[11 + i::23] = float("nan")
        a[US_ZERO_SLOT] = 0.0
        calls.append((a, idx, US_MARGINS[i]))
    return (hist, torch.full((US_SLOTS,), 99.0), scale, scale_inv, fmt_max), calls


# (R, C, want_t) of one fp8_quantize_weights call: C % 8 != 0; R % 8 != 0; R * C % 8 != 0; more than 65536
# elements (two amax blocks); 1 x 1; an all-zero weight (index WQ_ZERO); mixed want_t
WQ_WEIGHTS = [(72, 100, True), (100, 72, True), (7, 9, True), (264, 256, True), (1, 1, True), (16, 24, False),
              (65, 64, False), (128, 8, True)]
WQ_ZERO = 5
WQ_SLOTS = [9, 2, 14, 0, 5, 12, 3, 7]      # out of order, with unused slots between them
WQ_NSLOTS = 16


def wq_weights(dtype):
    g = R._gen(f"wq-{DT_NAME[dtype]}")
    ws = [(torch.randn(r, c, generator=g) * (0.02 * (i + 1))).to(dtype) for i, (r, c, _) in enumerate(WQ_WEIGHTS)]
    ws[WQ_ZERO].zero_()
    return ws


# ----------------------------------------------------------------------------
# fp8 GEMM: float64 reference and bound
# ----------------------------------------------------------------------------
def acc_units(K):
    """The accumulator term in units of 2**-24 cond (gemm_reference's own is K * 2**-23 cond = 2 K units)."""
    return ACC_HW + 2.0 * K / BK8


def alpha_of(alpha_a, alpha_b):
    return f32(f32(alpha_a) * f32(alpha_b))


def acc_ref(A8, B8, fa, fb, alpha):
    """(acc* = alpha A B^T, cond = |alpha| |A| |B|^T) in float64 on A8's device; A8 [M, K], B8 [N, K] codes."""
    a, b = decode(A8, fa), decode(B8, fb)
    return alpha * (a @ b.t()), abs(alpha) * (a.abs() @ b.abs().t())


def check_epilogue(epi, T, K, acc, cond, got_c, got_x, bias=None, aux=None, bdt=None, what="", tag=None, worst=None):
    """gemm_reference.check_epilogue with the fp8 accumulator term and the extra fp32 rounding of the staged
    value."""
    return R.check_epilogue(epi, T, acc_units(K) / 2.0, acc, cond, got_c, got_x, bias, aux, bdt, what, tag, worst, stage=E24)


def wgrad_slices(Rr, splits):
    nkt = Rr // BK8
    return [(s * nkt // splits, (s + 1) * nkt // splits) for s in range(splits)]


def wgrad_expected(A8, B8, fa, fb, alpha, splits, odt):
    """(ref, bound) of out[P, Q] = alpha A^T B from codes A8 [R, P], B8 [R, Q] through `splits` fp32 slabs."""
    a, b = decode(A8, fa), decode(B8, fb)
    Rr = a.shape[0]
    acc, cond = alpha * (a.t() @ b), abs(alpha) * (a.abs().t() @ b.abs())
    slab_abs = torch.zeros_like(acc)
    for kb, ke in wgrad_slices(Rr, splits):
        slab_abs += (alpha * (a[kb * BK8:ke * BK8].t() @ b[kb * BK8:ke * BK8])).abs()
    bound = acc_units(Rr) * E24 * cond + (splits + 1) * E24 * slab_abs + HALF_ULP[odt] * acc.abs() + TINY[odt]
    return acc, bound


def q8_expected(c_stored, q8_scale, q8_fmt, prev_amax=0.0):
    """(codes, amax) of the Q8 side output of a GEMM epilogue from the C it stored."""
    return quantize_ref(c_stored, q8_scale, q8_fmt), amax_ref(c_stored, prev_amax)


# ---- fp32 CPU emulation and its mutants ------------------------------------------------------------------
GEMM_MUTANTS = {
    # name: the class of cases it must be rejected on, a predicate over (epi, fa)
    "alpha_a_only": lambda e, fa: True,
    "alpha_after_rounding": lambda e, fa: e == "none",
    "e5m2_as_e4m3": lambda e, fa: fa == E5M2,
    "formats_swapped": lambda e, fa: fa == E5M2,
    "last_k128_dropped": lambda e, fa: True,
    "erf_tanh_swap": lambda e, fa: "gelu" in e,            # (gemm_reference's mutant, through the fp8 bound)
}


def emu_gemm(epi, T, A8, B8, fa, alpha_a, alpha_b, bias=None, aux=None, bdt=None, mut=None):
    """(C, X) of gemm_f8: fp32 accumulation of the decoded operands K-tile by K-tile, fl32(acc * alpha),
    then gemm_reference's epilogue emulation (which rounds the staged value to T first)."""
    fb = E4M3
    if mut == "e5m2_as_e4m3":
        fa = E4M3
    if mut == "formats_swapped":
        fa, fb = fb, fa
    a, b = decode(A8, fa).float(), decode(B8, fb).float()
    K = a.shape[1]
    if mut == "last_k128_dropped":
        K -= BK8
    acc = torch.zeros(a.shape[0], b.shape[0])
    for k0 in range(0, K, BK8):
        acc = acc + a[:, k0:k0 + BK8] @ b[:, k0:k0 + BK8].t()
    al = torch.tensor(alpha_a, dtype=torch.float32)
    if mut != "alpha_a_only":
        al = al * torch.tensor(alpha_b, dtype=torch.float32)
    staged = R._rnd(acc, T) * al if mut == "alpha_after_rounding" else acc * al
    return R.emu_epilogue(epi, T, staged, bias, aux, bdt, mut if mut in R.MUTANTS else None)


def emu_q8(c_stored, c_unrounded, q8_scale, q8_fmt, mut=None):
    """Q8 codes in fp32 arithmetic; mutant "q8_from_unrounded": from the fp32 value before its rounding to T."""
    src = c_unrounded if mut == "q8_from_unrounded" else c_stored
    return _emu_encode(src.float() * torch.tensor(q8_scale, dtype=torch.float32), q8_fmt, None)


def emu_wgrad(A8, B8, fa, fb, alpha, splits, odt):
    a, b = decode(A8, fa).float(), decode(B8, fb).float()
    al = torch.tensor(alpha, dtype=torch.float32)
    tot = torch.zeros(a.shape[1], b.shape[1])
    for kb, ke in wgrad_slices(a.shape[0], splits):
        slab = torch.zeros_like(tot)
        for t in range(kb, ke):
            slab = slab + a[t * BK8:(t + 1) * BK8].t() @ b[t * BK8:(t + 1) * BK8]
        tot = tot + slab * al
    return tot.to(odt)


# ----------------------------------------------------------------------------
# GEMM cases and seeded generators
# ----------------------------------------------------------------------------
Shape = R.Shape
# one full tile at one K-tile, the ping-pong pair, an odd count; edge tiles; a strided 2-D a, a batched 3-D a
NT_FULL = [Shape("full", 256, 256, k) for k in (128, 256, 384)]
NT_EDGE = [Shape("edge", m, n, k) for m, n, k in [(1, 8, 128), (8, 8, 128), (300, 392, 384), (257, 264, 256)]]
NT_LAYOUT = [Shape("layout", 256, 256, 128, "lda"), Shape("layout", 258, 264, 128, "a3d")]
NT_SHAPES = NT_FULL + NT_EDGE + NT_LAYOUT
Q8_SHAPES = [NT_FULL[0], NT_EDGE[2]]
Q8_EPIS = [e for e in R.EPIS if R.gelu_fwd(e) or R.colsum(e)]
Q8_ONLY_EPIS = ["bias_gelu_d", "bias_gelu_tanh_d", "mul"]
# weight-gradient form (R, P, Q, splits): one K-tile pair; uneven and even slices; a lone 16-column chunk each
# way; several partial tiles
WGRAD = [(128, 256, 256, 1), (384, 256, 256, 2), (384, 256, 256, 3), (256, 16, 272, 1), (256, 272, 16, 1),
         (640, 528, 272, 2)]
EXACT_ALPHA = (2.0, 0.5)     # a dropped alpha_a or alpha_b doubles or halves every integer


def persist_shape(cus, K):
    """A full-tile shape with eight more tiles than `cus` compute units (some workgroups walk two tiles)."""
    return Shape("persist", 256 * (cus // 4 + 2), 1024, K)


def dense_codes(name, rows, K, fmt):
    """Seeded codes [rows, K] across the whole format range: normal values scaled so that 4 sigma is the
    format's maximum (a few saturate, a few are subnormal), one element in 32 replaced by a uniformly drawn
    finite code, and the first row opened with +-max, the smallest subnormals and +-0."""
    g = R._gen(f"f8-{name}-{FMT_NAME[fmt]}")
    x = torch.randn(rows, K, generator=g) * (FMT_MAX[fmt] / 4)
    codes = encode(sat(x, fmt), fmt)
    any_code = torch.randint(0, MAX_CODE[fmt] + 1, (rows, K), generator=g).to(torch.uint8)
    any_code |= (torch.randint(0, 2, (rows, K), generator=g) << 7).to(torch.uint8)
    codes = torch.where(torch.rand(rows, K, generator=g) < 1 / 32, any_code, codes)
    head = torch.tensor([MAX_CODE[fmt], MAX_CODE[fmt] | 0x80, 0x01, 0x81, 0x00, 0x80, 0x02, 0x83], dtype=torch.uint8)
    codes[0, :8] = head
    return codes.contiguous()


def dense_alphas(K, fa):
    """Non-power-of-two inverse scales that bring the product of dense_codes operands to order one."""
    return f32(1.1 * 4.0 / FMT_MAX[fa] / math.sqrt(K)), f32(0.9 * 4.0 / FMT_MAX[E4M3])


def dense_code_operands(name, M, N, K, fa):
    """(A8 [M, K] in fa, B8 [N, K] e4m3, alpha_a, alpha_b), on the CPU."""
    return (dense_codes(f"{name}-a", M, K, fa), dense_codes(f"{name}-b", N, K, E4M3), *dense_alphas(K, fa))


def dense_bias_aux(name, M, N, T):
    """(bias [N], aux [M, N]) in T, seeded normal, on the CPU."""
    g = R._gen(f"f8-{name}-{DT_NAME[T]}")
    return torch.randn(N, generator=g).to(T), torch.randn(M, N, generator=g).to(T)


def dense_operands(name, M, N, K, fa, T):
    """(A8, B8, alpha_a, alpha_b, bias, aux): dense_code_operands and dense_bias_aux together."""
    return (*dense_code_operands(name, M, N, K, fa), *dense_bias_aux(name, M, N, T))


def phantom_last_column(A8, B8, bias, fa):
    """The Q8 amax trap of an edge tile, in place: the last row of B8 follows the signs of A8's first row at
    the largest magnitude, so acc[0, N - 1] is large, and bias[N - 1] cancels it. An edge tile stages the rows
    past N from row N - 1 and reads their bias from the last full chunk: its lanes past N hold that large
    sum under another bias, a value of no element of C that must not reach max |C|."""
    sign = torch.signbit(decode(A8[0], fa))
    B8[-1] = torch.where(sign, MAX_CODE[E4M3] | 0x80, MAX_CODE[E4M3]).to(torch.uint8)
    big = float((decode(A8[0], fa).abs() * FMT_MAX[E4M3]).sum()) * alpha_of(*dense_alphas(A8.shape[1], fa))
    bias[-1] = -1.125 * big
    return big


def dense_wgrad_operands(name, Rr, P, Q, fa):
    A8, B8 = dense_codes(f"wg-{name}-a", Rr, P, fa), dense_codes(f"wg-{name}-b", Rr, Q, E4M3)
    return (A8, B8, *dense_alphas(Rr, fa))


def exact_operands(M, N, K, fa):
    """gemm_reference.exact_operands (integers: A in {0, +-1, +-2}, B in [-8, 8], all exact in e4m3 and
    e5m2, nonzeros in every 64-deep K slice, no two rows or columns of the product alike) as codes, with the
    int64 originals: (A8, B8, A, B, bias, aux). With EXACT_ALPHA the kernel's alpha is exactly 1, so every
    partial sum, fl32(acc * alpha) and every epilogue result of gemm_reference.EXACT_EPIS is an integer that
    fp32, bf16 and fp16 hold exactly."""
    A, B, bias, aux = R.exact_operands(M, N, K)
    A8, B8 = encode(A, fa), encode(B, E4M3)
    assert torch.equal(decode(A8, fa), A.double()) and torch.equal(decode(B8, E4M3), B.double())
    return A8, B8, A, B, bias, aux
