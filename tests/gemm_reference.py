"""Float64 reference of the MFMA GEMM (csrc/gemm.hip and its three headers), the per-element error
bound its outputs are held to, an fp32 CPU emulation of every epilogue, and the shared test cases.

A plain helper module in the style of mt_reference.py / row_reference.py: no tests, no fixtures, and
it never calls the extension. tests/test_gemm_reference.py (fp32 emulation and its mutants against
this reference, on the CPU) and tests/test_gemm_numerics_gpu.py (the HIP kernels against it) share
the case tables and the seeded generators below, so both look at the same numbers.

References. Operands enter at their stored 16-bit values converted to double. acc* = A B^T (NT form)
or A^T B (weight-gradient form) exactly in float64, with its condition cond = |A| |B|^T. The
epilogues follow the header comment of gemm.hip and the rounding order written down in
gemm_epilogue.h: the accumulator is rounded to the operand dtype T (the LDS transposition), the
epilogue math runs in fp32, the result is rounded to T again. EPI_BIAS_GELU takes the GELU of the
stored (rounded) H; EPI_BIAS_GELU_D takes GELU and gelu' of the unrounded fp32 rnd_T(acc) + bias;
DGELU, MUL and the bias gradient work on the stored, rounded dh. Every function here runs on the
device of the tensors it is given: the persistent-kernel cases of the GPU test, whose shapes follow
the CU count, build acc* with a torch float64 product on the device, which is independent of the
kernel under test (the library's fp64 GEMM); everything else is computed on the CPU.

The bound, per element, with u = HALF_ULP[T] (derived here, not tuned):
  accumulator   delta = K * 2**-23 * cond. A product of two 16-bit values is exact in fp32; the K - 1
                additions are each off by at most one ulp (2**-23, which covers a rounding and a
                truncating accumulator alike) of a partial sum that |A| |B|^T bounds, in any order.
  staged value  rnd_T(acc): r1 = u |acc*| + delta.
  NONE          r1 + TINY.
  BIAS / RESID  ref = acc* + x: r1 + (u + 2**-23) |ref| + TINY (the fp32 add, the rounding to T).
  BIAS_GELU     H as BIAS. Y against the float64 GELU of the H the kernel stored: u |ref| + E_act(H) + TINY.
  BIAS_GELU_D   h* = acc* + bias is known to dh = r1 + 2**-23 |h*|. Y and G against gelu(h*) and
                gelu'(h*): sup |f'| over [h* - dh, h* + dh] times dh, plus E_act (E_g), plus
                u |ref| + TINY, where f' = gelu' (resp. gelu''). The sup is taken on the interval as
                |f'(h*)| + S2 dh with S2 = 2 >= sup |f''| for f in {gelu, gelu'} of both forms (pinned
                on a grid by the CPU test), so the bound stays tight in the tails where f' vanishes.
  DGELU / MUL   g = gelu'(aux) in float64, or aux: |g| r1 + |acc*| E_g + u |ref| + TINY, E_g = 0 for MUL.
  bias gradient against the float64 column sum of the dh the kernel stored:
                M * 2**-24 * sum_m |dh| + HALF_ULP[bdt] |ref| + TINY[bdt] (M fp32 additions in any order).
  weight grad   delta with K = R, plus splits * 2**-24 * sum_s |slab_s| for the slab combine, plus one
                rounding to the output dtype; gemm_tt_acc: ref = prev + acc*, and 2**-24 |ref| more.

E_act and E_g, the absolute error of the kernel's fp32 activation given its fp32 argument x, from
the kernel's own formulas (gemm_epilogue.h), all in units of 2**-24 = one fp32 rounding of a value
below 1:
  erf form, Phi(x) = 0.5 + sign(x) (0.5 - q), q = poly(t) t e, t = rcp(1 + p |x|), e = exp2(c x^2):
    - Abramowitz & Stegun 7.1.26 is within 1.5e-7 of erf, so within 0.75e-7 of Phi;
    - q <= 0.5 is a product of t (one FMA and one v_rcp, 1 ulp each), a five-term Horner polynomial
      (5 FMAs) and e (v_exp, 1 ulp): 8 ulp = 16 roundings relative, so 8 * 2**-24 absolute;
    - the argument of exp2 is c x^2 rounded three times, 3 * 2**-24 (x^2 / 2) relative on e; times q,
      and q x^2 / 2 <= 0.5 exp(-x^2/2) x^2 / 2 <= 0.19: under 1 * 2**-24;
    - the last add rounds once: 1 * 2**-24.
    E_PHI = 0.75e-7 + 10 * 2**-24, and gelu = x Phi is one more multiply:
    E_act(x) = |x| E_PHI + 2**-24 |gelu(x)|.
    gelu' = fma(x / sqrt(2 pi), e, Phi): Phi's error, the error of e times |x| pdf(x) <= 0.242 (1 ulp
    of v_exp, 1 ulp of the constant multiply: 0.97 * 2**-24) and |x|^3 pdf / 2 <= 0.231 times
    3 * 2**-24 (0.69 * 2**-24), one rounding of the result: E_g = E_PHI + 2**-24 (2 + |gelu'(x)|).
  tanh form, s = rcp(1 + exp2(-w log2 e)), w = 2 sqrt(2/pi) (x + 0.044715 x^3):
    - w carries 4 roundings; through exp that is 4 * 2**-24 |w| relative on the exponential, and
      s (1 - s) |w| <= |w| exp(-|w|) <= 0.37 of it on s: 1.5 * 2**-24;
    - v_exp (1 ulp) on the same path: s (1 - s) <= 0.25 of 2**-23: 0.5 * 2**-24;
    - the add and the v_rcp: 3 * 2**-24 of s <= 1.
    E_SIG = 6 * 2**-24 (5 rounded up), E_act(x) = |x| E_SIG + 2**-24 |gelu(x)|.
    gelu' = fma(x s (1 - s), w', s): s and s (1 - s) are each within E_SIG, the second multiplied by
    |x w'|; three roundings on the product and the result:
    E_g = E_SIG (1 + |x w'|) + 3 * 2**-24 (|x s (1 - s) w'| + |gelu'(x)|).
None of these was fitted to a GPU run.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass

import torch

from mt_reference import BF16, DT_NAME, F16, F32, HALF_ULP, TINY, f32  # noqa: F401

DTYPES = [BF16, F16]
INF = float("inf")
E23, E24 = 2.0 ** -23, 2.0 ** -24
BK = 64                       # the kernels' K-tile
E_PHI = 0.75e-7 + 10 * E24
E_SIG = 6 * E24
S2 = 2.0                      # >= sup |gelu''|, sup |gelu'''| of both forms
GELU_A, GELU_C = 0.044715, math.sqrt(2.0 / math.pi)
INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)

EPIS = ["none", "bias", "bias_gelu", "bias_gelu_tanh", "bias_gelu_d", "bias_gelu_tanh_d", "resid", "mul", "dgelu",
        "dgelu_tanh"]


def epi_attr(epi):            # the extension's constant for an epilogue name
    return "EPI_" + epi.upper()


def has_bias(e):
    return e.startswith("bias")


def aux_in(e):
    return e in ("resid", "mul", "dgelu", "dgelu_tanh")


def colsum(e):
    return e in ("mul", "dgelu", "dgelu_tanh")


def is_tanh(e):
    return "tanh" in e


def gelu_d(e):
    return e.endswith("_d")


def gelu_fwd(e):
    return e.startswith("bias_gelu")


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# ----------------------------------------------------------------------------
# float64 activations
# ----------------------------------------------------------------------------
def _tanh_parts(x):
    w = 2.0 * GELU_C * (x + GELU_A * x ** 3)
    s = torch.sigmoid(w)
    w1 = 2.0 * GELU_C * (1.0 + 3.0 * GELU_A * x * x)
    w2 = 12.0 * GELU_A * GELU_C * x
    return s, w1, w2


def phi64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def pdf64(x):
    return torch.exp(-0.5 * x * x) * INV_SQRT_2PI


def gelu64(x, tanh):
    if tanh:
        return x * _tanh_parts(x)[0]
    return x * phi64(x)


def dgelu64(x, tanh):
    if tanh:
        s, w1, _ = _tanh_parts(x)
        return s + x * s * (1.0 - s) * w1
    return phi64(x) + x * pdf64(x)


def d2gelu64(x, tanh):
    if tanh:
        s, w1, w2 = _tanh_parts(x)
        q = s * (1.0 - s)
        return 2.0 * q * w1 + x * q * ((1.0 - 2.0 * s) * w1 * w1 + w2)
    return pdf64(x) * (2.0 - x * x)


def e_act(x, tanh):
    """|kernel gelu(x) - gelu(x)| for an fp32 x (module docstring)."""
    return x.abs() * (E_SIG if tanh else E_PHI) + E24 * gelu64(x, tanh).abs()


def e_g(x, tanh):
    """|kernel gelu'(x) - gelu'(x)| for an fp32 x (module docstring)."""
    g = dgelu64(x, tanh).abs()
    if tanh:
        s, w1, _ = _tanh_parts(x)
        return E_SIG * (1.0 + (x * w1).abs()) + 3 * E24 * ((x * s * (1.0 - s) * w1).abs() + g)
    return E_PHI + E24 * (2.0 + g)


# ----------------------------------------------------------------------------
# comparison
# ----------------------------------------------------------------------------
WORST = {}   # tag -> (largest ratio seen by check, case)


def ratio(got, ref, bound):
    """(worst |got - ref| / bound, its index), on ref's device; inf where got is not finite."""
    got = got.detach().to(ref.device).double()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if not got.numel():
        return 0.0, ()
    r = (got - ref).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, INF))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape))


def check(got, ref, bound, what="", tag=None):
    """Assert |got - ref| <= bound on every element; returns the worst ratio."""
    worst, idx = ratio(got, ref, bound)
    if tag is not None and worst > WORST.get(tag, (-1.0, ""))[0]:
        WORST[tag] = (worst, what)
    if worst > 1.0:
        g = got.detach().to(ref.device).double()[idx]
        raise AssertionError(f"{what}: worst |got - ref| / bound = {worst:.4g} at {idx}: got {float(g)!r}, "
                             f"ref {float(ref[idx])!r}, bound {float(bound[idx])!r}")
    return worst


# ----------------------------------------------------------------------------
# float64 references and bounds
# ----------------------------------------------------------------------------
def acc_ref(A, B):
    """(acc* = A B^T, cond = |A| |B|^T) in float64 on A's device, A [M, K], B [N, K]."""
    a, b = A.double(), B.double()
    return a @ b.t(), a.abs() @ b.abs().t()


def expected(epi, T, K, acc, cond, bias=None, aux=None, got=None, stage=0.0):
    """The outputs of one epilogue as {name: (ref, bound)}: "C", and "X" (H of BIAS_GELU, G of BIAS_GELU_D).
    bias [N] and aux [M, N] at their stored values; ``got`` = {"X": the H the kernel stored} is needed by
    BIAS_GELU, whose Y is held to the GELU of that H. ``stage``: the relative error of an fp32 operation on the
    accumulator before its rounding to T (0 for the 16-bit kernels; the fp8 kernels' alpha multiply, 2**-24:
    tests/fp8_reference.py)."""
    u, tiny = HALF_ULP[T], TINY[T]
    delta = K * E23 * cond
    r1 = (u + stage) * acc.abs() + delta
    tanh = is_tanh(epi)
    if epi == "none":
        return {"C": (acc, r1 + tiny)}
    if epi in ("bias", "resid"):
        ref = acc + (bias.double()[None, :] if epi == "bias" else aux.double())
        return {"C": (ref, r1 + (u + E23) * ref.abs() + tiny)}
    if epi in ("bias_gelu", "bias_gelu_tanh"):
        h = acc + bias.double()[None, :]
        hs = got["X"].detach().to(acc.device).double().reshape(acc.shape)
        y = gelu64(hs, tanh)
        return {"X": (h, r1 + (u + E23) * h.abs() + tiny), "C": (y, u * y.abs() + e_act(hs, tanh) + tiny)}
    if gelu_d(epi):
        h = acc + bias.double()[None, :]
        dh = r1 + E23 * h.abs()
        y, g = gelu64(h, tanh), dgelu64(h, tanh)
        by = (g.abs() + S2 * dh) * dh + e_act(h, tanh) + u * y.abs() + tiny
        bg = (d2gelu64(h, tanh).abs() + S2 * dh) * dh + e_g(h, tanh) + u * g.abs() + tiny
        return {"C": (y, by), "X": (g, bg)}
    x = aux.double()
    if epi == "mul":
        g, eg = x, 0.0
    else:
        g, eg = dgelu64(x, tanh), e_g(x, tanh)
    ref = acc * g
    return {"C": (ref, g.abs() * r1 + acc.abs() * eg + u * ref.abs() + tiny)}


def bias_grad_expected(dh_stored, bdt):
    """(ref, bound) of the bias gradient from the dh the kernel stored ([M, N], any leading shape)."""
    dh = dh_stored.detach().double().reshape(-1, dh_stored.shape[-1])
    ref = dh.sum(0)
    return ref, dh.shape[0] * E24 * dh.abs().sum(0) + HALF_ULP[bdt] * ref.abs() + TINY[bdt]


def check_epilogue(epi, T, K, acc, cond, got_c, got_x, bias=None, aux=None, bdt=None, what="", tag=None, worst=None,
                   stage=0.0):
    """Hold every output of one GEMM call to its bound. got_c: C; got_x: H / G / the bias gradient (dtype bdt).
    ``worst`` (a dict) collects ratios instead of asserting (the mutant tests). Returns the largest ratio."""
    exp = expected(epi, T, K, acc, cond, bias, aux, {"X": got_x} if gelu_fwd(epi) and not gelu_d(epi) else None, stage)
    outs = [("C", got_c.reshape(acc.shape), *exp["C"])]
    if "X" in exp:
        outs.append(("X", got_x.reshape(acc.shape), *exp["X"]))
    if colsum(epi) and bdt is not None:
        outs.append(("dbias", got_x, *(t.to(acc.device) for t in bias_grad_expected(got_c.to(acc.device), bdt))))
    top = 0.0
    for name, g, ref, bound in outs:
        assert g.dtype == (bdt if name == "dbias" else T), (name, g.dtype)
        if worst is not None:
            r = ratio(g, ref, bound)[0]
            worst[name] = max(worst.get(name, 0.0), r)
        else:
            dn = DT_NAME[T] + ("/db-" + DT_NAME[bdt] if name == "dbias" else "")
            r = check(g, ref, bound, f"{what} {epi} {name}", None if tag is None else f"{tag} {epi} {name} {dn}")
        top = max(top, r)
    return top


def wgrad_slices(R, splits):
    """K-tile ranges [kb, ke) of the split-K slices (gemm_nt_kernel, TR)."""
    nkt = R // BK
    return [(s * nkt // splits, (s + 1) * nkt // splits) for s in range(splits)]


def wgrad_expected(A, B, splits, odt, prev=None):
    """(ref, bound) of out[P, Q] = A^T B (+ prev), A [R, P], B [R, Q], through `splits` fp32 slabs, in odt."""
    a, b = A.double(), B.double()
    R = a.shape[0]
    acc, cond = a.t() @ b, a.abs().t() @ b.abs()
    slab_abs = torch.zeros_like(acc)
    for kb, ke in wgrad_slices(R, splits):
        slab_abs += (a[kb * BK:ke * BK].t() @ b[kb * BK:ke * BK]).abs()
    ref = acc if prev is None else acc + prev.double()
    bound = R * E23 * cond + splits * E24 * slab_abs + HALF_ULP[odt] * ref.abs() + TINY[odt]
    if prev is not None:
        bound = bound + E24 * ref.abs()
    return ref, bound


# ----------------------------------------------------------------------------
# fp32 CPU emulation (the correct implementation the bound must admit) and its mutants
# ----------------------------------------------------------------------------
MUTANTS = {
    # name: the class of cases it must be rejected on (a predicate over (epi, dtype, M, N, K))
    "bias_shift_chunk": lambda e, T, M, N, K: has_bias(e) and N > 8,
    "bias_drop_last_chunk": lambda e, T, M, N, K: has_bias(e) and N % 256 != 0,
    "erf_tanh_swap": lambda e, T, M, N, K: "gelu" in e,
    "deriv_phi_only": lambda e, T, M, N, K: gelu_d(e),
    "ktile_dropped_in_fragment": lambda e, T, M, N, K: M >= 32 and N >= 32,
    "ktile_mispaired": lambda e, T, M, N, K: K >= 2 * BK,
    "fragment_transposed": lambda e, T, M, N, K: M >= 32 and N >= 48,
    "acc_rounded_per_ktile": lambda e, T, M, N, K: K >= 2 * BK,
    "f16_through_bf16": lambda e, T, M, N, K: T == F16,
    "bgrad_rows_past_m": lambda e, T, M, N, K: e in ("dgelu", "dgelu_tanh") and M % 256 != 0,
    "bgrad_second_wave_missing": lambda e, T, M, N, K: colsum(e) and M > 128,
    "resid_ld_plus_8": lambda e, T, M, N, K: e == "resid" and M > 1,
}
WGRAD_MUTANTS = ["slab_dropped", "slice_boundary_off_by_one"]   # class: splits > 1


def _rnd(x, T):
    return x.to(T).float()


def emu_acc(A, B, T, mut=None):
    """fp32 accumulator of A B^T, K-tile by K-tile."""
    M, K = A.shape
    N = B.shape[0]
    nt = K // BK
    a, b = A.float(), B.float()
    acc = torch.zeros(M, N)
    for t in range(nt):
        tb = (t + 1) % nt if mut == "ktile_mispaired" else t
        part = a[:, t * BK:(t + 1) * BK] @ b[:, tb * BK:(tb + 1) * BK].t()
        if mut == "ktile_dropped_in_fragment" and t == nt - 1:
            part[16:32, 16:32] = 0.0
        acc = acc + part
        if mut == "acc_rounded_per_ktile":
            acc = _rnd(acc, T)
    if mut == "fragment_transposed":
        acc[16:32, 32:48] = acc[16:32, 32:48].t().clone()
    return acc


def emu_cdf(x, e):
    """Phi(x) as gemm_epilogue.h cdf2 evaluates it (A&S 7.1.26, constants folded), fp32."""
    c = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    ax = x.abs()
    t = 1.0 / (c(0.3275911) * c(0.70710678118654752) * ax + 1.0)
    p = c(0.5) * c(1.061405429) * t + c(0.5) * c(-1.453152027)
    p = p * t + c(0.5) * c(1.421413741)
    p = p * t + c(0.5) * c(-0.284496736)
    p = p * t + c(0.5) * c(0.254829592)
    r = (-p * t) * e + 0.5
    return 0.5 + torch.copysign(r, x)


def emu_gelu_and_grad(x, tanh, mut=None):
    """(gelu(x), gelu'(x)) in fp32 by the kernel's formulas."""
    assert x.dtype == torch.float32
    c = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    if tanh:
        u = c(-2.0 * 0.7978845608028654 * 1.4426950408889634) * (c(0.044715) * x * (x * x) + x)
        sg = 1.0 / (1.0 + torch.exp2(u))
        du = c(2.0 * 0.7978845608028654) * (c(3.0 * 0.044715) * x * x + 1.0)
        g = sg if mut == "deriv_phi_only" else (x * sg * (1.0 - sg)) * du + sg
        return x * sg, g
    e = torch.exp2(c(-0.72134752044448170) * x * x)
    cdf = emu_cdf(x, e)
    g = cdf if mut == "deriv_phi_only" else (x * c(0.39894228040143268)) * e + cdf
    return x * cdf, g


def emu_epilogue(epi, T, acc32, bias=None, aux=None, bdt=None, mut=None):
    """(C, X) of one epilogue from the fp32 accumulator, with the kernel's rounding points. X: H, G or the
    bias gradient (in bdt, summed from per-(256-row tile, 128-row wave) fp32 partials of the stored dh)."""
    M, N = acc32.shape
    tanh = is_tanh(epi) != (mut == "erf_tanh_swap")
    out_T = (lambda v: v.to(BF16).to(T)) if mut == "f16_through_bf16" else (lambda v: v.to(T))
    r = _rnd(acc32, T)
    if has_bias(epi):
        b = bias.float()
        if mut == "bias_shift_chunk":
            b = torch.roll(b, -8)
        if mut == "bias_drop_last_chunk":
            b = b.clone()
            b[-8:] = 0.0
    if epi == "none":
        return out_T(r), None
    if epi == "bias":
        return out_T(r + b), None
    if epi == "resid":
        x = aux.float()
        if mut == "resid_ld_plus_8":
            flat = torch.cat([x.reshape(-1), torch.zeros(8 * M)])
            x = flat[:M * (N + 8)].view(M, N + 8)[:, :N]
        return out_T(r + x), None
    if gelu_fwd(epi):
        v = r + b
        if gelu_d(epi):
            y, g = emu_gelu_and_grad(v, tanh, mut)
            return out_T(y), out_T(g)
        h = out_T(v)
        return out_T(emu_gelu_and_grad(h.float(), tanh)[0]), h
    x = aux.float()
    g = x if epi == "mul" else emu_gelu_and_grad(x, tanh)[1]
    c = out_T(r * g)
    if bdt is None:
        return c, None
    pad = (-M) % 256
    st = torch.cat([c.float(), torch.zeros(pad, N)])
    if mut == "bgrad_rows_past_m" and pad:
        g0 = emu_gelu_and_grad(torch.zeros(1), tanh)[1]   # the out-of-range aux reads 0
        st[M:] = out_T(r[M - 1:M] * g0).float()
    parts = st.view(-1, 128, N).sum(1)
    if mut == "bgrad_second_wave_missing":
        parts = torch.cat([parts[:1], parts[2:]])
    return c, parts.sum(0).to(bdt)


def emu_gemm(epi, T, A, B, bias=None, aux=None, bdt=None, mut=None):
    return emu_epilogue(epi, T, emu_acc(A, B, T, mut), bias, aux, bdt, mut)


def emu_wgrad(A, B, splits, odt, prev=None, mut=None):
    """out[P, Q] = A^T B (+ prev) through fp32 slabs of whole K-tiles, combined in fp32, rounded to odt."""
    a, b = A.float(), B.float()
    sl = wgrad_slices(a.shape[0], splits)
    if mut == "slice_boundary_off_by_one":
        sl[0] = (sl[0][0], sl[0][1] + 1)
    if mut == "slab_dropped":
        sl = sl[:-1]
    tot = torch.zeros(a.shape[1], b.shape[1]) if prev is None else prev.float().clone()
    for kb, ke in sl:
        slab = torch.zeros_like(tot)
        for t in range(kb, ke):
            slab = slab + a[t * BK:(t + 1) * BK].t() @ b[t * BK:(t + 1) * BK]
        tot = tot + slab
    return tot.to(odt)


# ----------------------------------------------------------------------------
# cases and seeded generators
# ----------------------------------------------------------------------------
@dataclass(frozen=True)
class Shape:
    path: str      # "full", "edge", "layout", "persist"
    M: int
    N: int
    K: int
    layout: str = "plain"   # "lda", "ldb", "a3d", "offset16"
    epis: tuple = tuple(EPIS)

    @property
    def name(self):
        return f"{self.path}-{self.M}x{self.N}x{self.K}" + ("" if self.layout == "plain" else "-" + self.layout)


# one tile per workgroup, full tiles: one, two, three K-tiles, the pair loop with and without an odd tail;
# several tiles; nine tile rows (last GROUP_M panel of height 1, 18 tiles: an XCD-remap remainder); a deep K
FULL = [Shape("full", 256, 256, k) for k in (64, 128, 192, 256, 320)] + [
    Shape("full", 512, 768, 128), Shape("full", 2304, 512, 64), Shape("full", 256, 512, 1024)]
# edge kernel: a partial 8-row slot (77, 300), a partial 64-row half (77, 300), an empty second wave row
# (1, 77, 300's second tile), a lone extra row (1, 129, 257), a lone 8-column chunk (8, 72, 200, 264, 520)
EDGE = [Shape("edge", m, n, k) for m, n, k in
        [(1, 264, 64), (77, 8, 128), (129, 72, 192), (255, 200, 64), (257, 264, 128), (300, 520, 192),
         (300, 200, 64), (129, 520, 128), (300, 200, 1024)]]
LAYOUT = [Shape("layout", m, n, 128, lay) for m, n in [(256, 256), (258, 264)]
          for lay in ("lda", "ldb", "a3d", "offset16")]
NT_SHAPES = FULL + EDGE


def persist_shapes(cus):
    """Persistent-kernel shapes for a device with `cus` compute units: eight more tiles than CUs (some
    workgroups walk two tiles, most one) with every epilogue, and one three-tiles-per-workgroup shape."""
    two = [Shape("persist", 256 * (cus // 4 + 2), 1024, k) for k in (64, 128, 192)]
    three = Shape("persist", 256 * (cus // 2 + 2), 1024, 128, epis=("none", "bias_gelu_d", "mul"))
    return two + [three]


# weight-gradient form: (R, P, Q, splits)
WGRAD_PQ = [(256, 256), (200, 264), (8, 1608), (520, 256)]
WGRAD = [(r, p, q, s) for r in (64, 192, 320, 448) for (p, q) in WGRAD_PQ for s in (1, 3, 5) if r // BK >= s]
TRANSPOSE_SHAPES = [(8, 8), (1, 64), (1000, 33), (264, 72), (520, 256)]


def dense_operands(name, M, N, K, T):
    """Seeded normal operands: A / sqrt(K) [M, K], B [N, K], bias [N], aux [M, N], all in T, on the CPU."""
    g = _gen(f"{name}-{DT_NAME[T]}")
    A = (torch.randn(M, K, generator=g) / math.sqrt(K)).to(T)
    B = torch.randn(N, K, generator=g).to(T)
    bias = torch.randn(N, generator=g).to(T)
    aux = torch.randn(M, N, generator=g).to(T)
    return A, B, bias, aux


def dense_wgrad_operands(name, R, P, Q, T):
    g = _gen(f"wgrad-{name}-{DT_NAME[T]}")
    return (torch.randn(R, P, generator=g) / math.sqrt(R)).to(T), torch.randn(R, Q, generator=g).to(T)


EXACT_NNZ = 8                                  # nonzeros per row of the exact A
_EXACT_VAL = torch.tensor([1, -1, 2, -2])      # a base-4 digit of m -> the nonzero's value


def _exact_cols(M, K):
    """Columns and values of the EXACT_NNZ nonzeros of every row of the exact A: nonzero j of row m has
    the value of m's j-th base-4 digit (so no two of the first 4**8 rows carry the same values) and sits in
    K-tile (m + j) mod (K / 64) — with at most eight K-tiles every row touches each of them, with more, every
    eight consecutive tiles — at an offset inside the tile that moves with j, m and m // 64."""
    m = torch.arange(M)
    nt = K // BK
    ks, vs = [], []
    for j in range(EXACT_NNZ):
        off = (11 * j + 5 * (m // nt) + 3 * (m // 64)) % BK   # (11 j mod 64 differ: one row's columns are distinct)
        ks.append(((m + j) % nt) * BK + off)
        vs.append(_EXACT_VAL[(m // 4 ** j) % 4])
    return ks, vs


def exact_acc(A, B):
    """A B^T in int64 for exact_operands' A (eight nonzeros per row): eight gathered rows of B^T per row of A,
    which is A @ B.t() (tests/test_gemm_reference.py checks that) without an int64 matrix product."""
    ks, vs = _exact_cols(*A.shape)
    bt = B.t().contiguous()
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=torch.int64)
    for k, v in zip(ks, vs):
        acc += v[:, None] * bt[k]
    return acc


def exact_operands(M, N, K):
    """Integer-valued operands (int64) whose every partial sum and result is an integer of magnitude <= 256,
    so every order of accumulation and every rounding is exact in bf16 and fp16. A: _exact_cols. B[n, k] =
    ((3n + 5k + (n // 17)(k mod 13) + (n // 289)(k mod 11)) mod 17) - 8: no two rows of B alike. bias in
    [-8, 8] moves with n, aux in [-2, 2] with (m, n). |acc| <= 8 * 2 * 8 = 128, |acc + bias| <= 136,
    |acc * aux| <= 256, and a column of the multiply sums exactly in fp32. tests/test_gemm_reference.py
    asserts for every shape of the tables that all rows of acc differ from each other, and all columns
    (where there are at least 64 rows to tell them apart), so a result written to the wrong row, 8-row
    slot, 64-row half, 128-row wave tile, 256-row tile or column chunk is a wrong integer; and that
    every K-tile of A and of B carries nonzeros."""
    m = torch.arange(M)
    ks, vs = _exact_cols(M, K)
    A = torch.zeros(M, K, dtype=torch.int64)
    for k, v in zip(ks, vs):
        A[m, k] = v
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    B = (3 * n + 5 * k + (n // 17) * (k % 13) + (n // 289) * (k % 11)) % 17 - 8
    bias = (5 * torch.arange(N)) % 17 - 8
    aux = (2 * m[:, None] + 3 * torch.arange(N)[None, :]) % 5 - 2
    return A, B, bias, aux


def exact_expected(epi, A, B, bias, aux):
    """int64 results of the epilogues that are exact on exact_operands: {"C": ..} plus "X" (H of BIAS_GELU) or
    "dbias" (MUL)."""
    acc = exact_acc(A, B)
    if epi == "none":
        return {"C": acc}
    if epi == "bias":
        return {"C": acc + bias[None, :]}
    if epi == "resid":
        return {"C": acc + aux}
    if epi == "mul":
        c = acc * aux
        return {"C": c, "dbias": c.sum(0)}
    if epi == "bias_gelu":
        return {"X": acc + bias[None, :]}
    raise AssertionError(epi)


EXACT_EPIS = ["none", "bias", "resid", "mul", "bias_gelu"]
