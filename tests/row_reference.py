"""Float64 reference of the row kernels (csrc/softmax.hip, csrc/xentropy.hip, csrc/layer_norm.hip),
the error bound they are held to, and the shared test cases.

A plain helper module in the style of mt_reference.py: no tests, no fixtures. It holds

* straight float64 PyTorch-on-CPU implementations of the scale-mask softmax (forward, and backward
  from the *stored* y), the label-smoothed softmax cross-entropy (lse, loss, dlogits) and
  LayerNorm / RMSNorm (y, mean, rstd, dx, dgamma, dbeta), written from the formulas in the kernel
  header comments. They never call the extension. Inputs enter at their stored (16-bit or fp32)
  values converted to double; scale, eps and smoothing are rounded to fp32 once (mt_reference.f32)
  and the same value goes to the reference, the fp32 CPU formulation and the kernel;
* for every output its `cond`: the sum of the absolute values of the terms its formula adds, in
  float64. An fp32 evaluation of the formula cannot be closer to the exact result than a few ulp
  of cond, however it orders its work, and a correct one is not much further away;
* check(got, ref, cond, dtype): every element satisfies

      |got - ref| <= HALF_ULP[dtype] * |ref| + C * cond + TINY[dtype]

  HALF_ULP * |ref| is the one rounding to the output dtype, TINY its subnormal step. C = 2**-16
  is the allowance for the fp32 pipeline before that rounding, derived and not measured:
    - __expf / __logf scale their argument by log2(e) / ln(2) in fp32 before the hardware
      exp2 / log2 (1 ulp each): an argument a carries a * 2**-23 of absolute error, which is the
      relative error of exp(a). The arguments here are row-max-subtracted scores and x - lse,
      |a| <= 88 before exp underflows in fp32: 88 * 2**-23 = 2**-16.5;
    - at most 64 sequential fp32 adds per lane (softmax KPL 8 x 8 elements), then a 6-step
      butterfly and at most 4 waves: (64 + 6 + 4) * 2**-24 = 2**-17.8 of cond;
    - one divide or rsqrt (2 ulp): 2**-23.
  The first two do not reach their worst case on the same element (a score 88 below the row
  maximum has a weight of e**-88 in the sums), so C = 2**-16 covers them. For the 16-bit outputs
  C is 1/32 (fp16) and 1/256 (bf16) of the rounding term wherever cond is of the size of |ref|,
  so the check still tells one rounding from two. C was not re-derived for any case.
  One cond was: dgamma. With cond = sum_rows |dy xhat|, which takes xhat as given, the fp32 CPU
  formulation (F.layer_norm, a correct implementation) is outside the bound on four cases:
  ln/f32-wf32-r1-c1032 1.35, ln/f16-wf32-r1-c2056 1.14, ln/f16-wf32-r1-c5000 1.73 and
  ln/f32-wf32-r5-c512-shift100 1.50 times the bound. xhat is itself a difference the formula
  evaluates, x rstd - mean rstd, and carries 2**-24 rstd (|x| + |mean|) of error however small it
  comes out: with one row, a column where x is near the mean has a dgamma of almost nothing and no
  C covers it; with x + 100 every column loses 200 / |xhat| in relative terms. No constant fixes
  that, so dgamma's cond counts the two terms of xhat, as y's cond does:
  sum_rows |dy| rstd (|x| + |mean|). For RMSNorm (mean = 0) that is sum_rows |dy xhat| again.
* BOUNDS: for the fp32-valued per-row scalars (lse, loss, mean, rstd) the measured error of the
  package's own fp32 CPU formulation (softmax_xentropy on CPU tensors, F.layer_norm's statistics,
  _ref_rms) against this reference, per case. The GPU tests allow MARGIN (4) times that plus
  SCALAR_FAST = 2**-20 * max(1, |ref|) for the fast log / exp / rsqrt;
* the case tables and seeded input generators that tests/test_row_reference.py (fp32 CPU
  formulations and mutants against this reference) and tests/test_row_kernels_gpu.py (HIP kernels
  against this reference) share, so both look at the same numbers.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import torch

from mt_reference import BF16, DT_NAME, F16, F32, HALF_ULP, MARGIN, TINY, f32  # noqa: F401

DTYPES = [F32, F16, BF16]
C = 2.0 ** -16
SCALAR_FAST = 2.0 ** -20
assert C <= HALF_ULP[F16] / 8

INF = float("inf")


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# ----------------------------------------------------------------------------
# comparison
# ----------------------------------------------------------------------------
WORST = {}   # tag -> (largest ratio seen by check, case); the GPU tests report it per kernel and dtype


def ratio(got, ref, cond, dtype):
    """(worst |got - ref| / bound, its index); inf where got is not finite."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape == cond.shape, (got.shape, ref.shape, cond.shape)
    if not got.numel():
        return 0.0, ()
    tol = HALF_ULP[dtype] * ref.abs() + C * cond + TINY[dtype]
    r = (got - ref).abs() / tol
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, INF))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape))


def check(got, ref, cond, dtype, what="", tag=None):
    """Assert the bound of the module docstring on every element; returns the worst ratio."""
    worst, idx = ratio(got, ref, cond, dtype)
    if tag is not None and worst > WORST.get(tag, (-1.0, ""))[0]:
        WORST[tag] = (worst, what)
    if worst > 1.0:
        g = got.detach().cpu().double()[idx]
        raise AssertionError(f"{what}: worst |got - ref| / bound = {worst:.4g} at {idx}: got {float(g)!r}, "
                             f"ref {float(ref[idx])!r}, cond {float(cond[idx])!r} ({DT_NAME[dtype]})")
    return worst


def scalar_excess(got, ref, bound):
    """max over rows of |got - ref| / (MARGIN * bound + SCALAR_FAST * max(1, |ref|)) for an fp32 scalar."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not got.numel():
        return 0.0
    tol = MARGIN * bound + SCALAR_FAST * ref.abs().clamp(min=1.0)
    r = (got - ref).abs() / tol
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, INF))
    return float(r.max())


def max_err(got, ref) -> float:
    if not ref.numel():
        return 0.0
    d = (got.detach().cpu().double() - ref).abs()
    assert bool(torch.isfinite(d).all()), "non-finite value in result"
    return float(d.max())


# ----------------------------------------------------------------------------
# float64 references
# ----------------------------------------------------------------------------
def ref_softmax_fwd(x, scale, mode, mask=None):
    """y = softmax(s) over the last dim of x [b, h, sq, sk], s = x * scale; mode "mask": s = -10000
    where the byte mask [b, 1|h, sq, sk] is nonzero; mode "causal": s = -inf (an exact 0) where
    key > query. A row without a finite score gives zeros. Returns (y, cond = |y|)."""
    s = x.double() * float(scale)
    sq, sk = s.shape[-2:]
    if mode == "mask":
        s = torch.where(mask.bool().expand(s.shape), torch.full_like(s, -10000.0), s)
    elif mode == "causal":
        key, qry = torch.arange(sk)[None, :], torch.arange(sq)[:, None]
        s = torch.where((key > qry).expand(s.shape), torch.full_like(s, -INF), s)
    else:
        assert mode == "none", mode
    m = s.max(-1, keepdim=True).values
    e = torch.where(s == -INF, torch.zeros_like(s), (s - torch.where(m == -INF, torch.zeros_like(m), m)).exp())
    z = e.sum(-1, keepdim=True)
    y = torch.where(z > 0, e / z, torch.zeros_like(e))
    return y, y.abs()


def ref_softmax_bwd(dy, y, scale):
    """dx = scale * y * (dy - sum(dy * y)) from the stored y. Returns (dx, cond)."""
    dy, y, scale = dy.double(), y.double(), float(scale)
    dot = (dy * y).sum(-1, keepdim=True)
    dx = scale * y * (dy - dot)
    cond = abs(scale) * y.abs() * (dy.abs() + (dy * y).abs().sum(-1, keepdim=True))
    return dx, cond


def xent_valid(labels, V, ignore_index):
    """Rows that count: an ignored or out-of-range label gives loss 0 and grad 0."""
    return (labels != ignore_index) & (labels >= 0) & (labels < V)


def ref_xent(x, labels, smoothing, ignore_index, g=None):
    """lse, loss = (1-s)(lse - x_y) + s (lse - mean x) and, with the per-row loss gradient g,
    dlogits = g (softmax(x) - (1-s) onehot(y) - s/V) with its cond. Without smoothing sum(x) stays
    out of the loss (it is -inf for a row with masked columns)."""
    x = x.double()
    N, V = x.shape
    s = float(smoothing)
    valid = xent_valid(labels, V, ignore_index)
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    lse = torch.logsumexp(x, -1)
    xy = x.gather(1, safe[:, None]).squeeze(1)
    loss = (1.0 - s) * (lse - xy)
    if s != 0.0:
        loss = loss + s * (lse - x.mean(-1))
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    out = {"lse": lse, "loss": loss, "valid": valid}
    if g is not None:
        gv = torch.where(valid, g.double(), torch.zeros(N, dtype=torch.float64))[:, None]
        p = (x - lse[:, None]).exp()
        onehot = torch.zeros_like(x)
        onehot[torch.arange(N), safe] = 1.0
        out["dlogits"] = gv * (p - (1.0 - s) * onehot - s / V)
        out["dlogits_cond"] = gv.abs() * (p + s / V + (1.0 - s) * onehot)
    return out


def ref_norm_fwd(x, gamma, beta, eps, rms):
    """x [rows, cols] -> dict(y, y_cond, mean, rstd, xhat). LayerNorm: xhat = (x - mean) rstd,
    rstd = 1 / sqrt(var + eps) with the biased variance; RMSNorm: mean = 0, rstd = 1 / sqrt(mean(x^2)
    + eps). y = xhat gamma + beta (gamma = 1 / beta = 0 when absent)."""
    x = x.double()
    rows, cols = x.shape
    mean = torch.zeros(rows, 1, dtype=torch.float64) if rms else x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / (var + float(eps)).sqrt()
    xhat = (x - mean) * rstd
    g = gamma.double().reshape(1, cols) if gamma is not None else torch.ones(1, cols, dtype=torch.float64)
    b = beta.double().reshape(1, cols) if beta is not None else torch.zeros(1, cols, dtype=torch.float64)
    y = xhat * g + b
    cond = g.abs() * rstd * (x.abs() + mean.abs()) + b.abs()
    return {"y": y, "y_cond": cond, "mean": mean.squeeze(1), "rstd": rstd.squeeze(1), "xhat": xhat, "g": g,
            "xhat_cond": rstd * (x.abs() + mean.abs())}


def ref_norm_bwd(dy, fwd, rms):
    """From ref_norm_fwd's own float64 statistics: dx = rstd (dy g - s1 - xhat s2), s1 = mean(dy g)
    (0 for RMSNorm), s2 = mean(dy g xhat); dgamma = sum_rows dy xhat; dbeta = sum_rows dy.
    dgamma's cond counts xhat = x rstd - mean rstd as the two terms it is (module docstring)."""
    dy = dy.double()
    xhat, g, rstd = fwd["xhat"], fwd["g"], fwd["rstd"][:, None]
    dyg = dy * g
    s1 = torch.zeros_like(rstd) if rms else dyg.mean(-1, keepdim=True)
    s2 = (dyg * xhat).mean(-1, keepdim=True)
    dx = rstd * (dyg - s1 - xhat * s2)
    a1 = torch.zeros_like(rstd) if rms else dyg.abs().mean(-1, keepdim=True)
    dx_cond = rstd * (dyg.abs() + a1 + xhat.abs() * (dyg * xhat).abs().mean(-1, keepdim=True))
    return {"dx": dx, "dx_cond": dx_cond,
            "dgamma": (dy * xhat).sum(0), "dgamma_cond": (dy.abs() * fwd["xhat_cond"]).sum(0),
            "dbeta": dy.sum(0), "dbeta_cond": dy.abs().sum(0)}


# ----------------------------------------------------------------------------
# softmax cases
# ----------------------------------------------------------------------------
# every KPL (<= 512, 1024, 2048, 4096 columns) and both sides of each boundary
SMX_SK = [8, 64, 504, 512, 520, 1024, 1032, 2048, 2056, 3000, 4096]
SMX_MODES = ["none", "mask1", "maskh", "causal"]   # mask1: [b, 1, sq, sk]; maskh: [b, h, sq, sk]
SMX_SCALES = [1.0, 0.125]


@dataclass(frozen=True)
class SmxCase:
    name: str
    dtype: torch.dtype
    b: int
    h: int
    sq: int
    sk: int
    scale: float
    mode: str
    neginf: bool = False

    @property
    def kernel_mode(self):
        return "mask" if self.mode.startswith("mask") else self.mode


def _smx_cases():
    out = {}
    for dt in DTYPES:
        for i, sk in enumerate(SMX_SK):
            for j, mode in enumerate(SMX_MODES):
                # rows = b h sq = 3, 6, 21 or 42: never a multiple of the 4 rows of a block
                b, h = (1, 3) if mode in ("none", "causal") else (2, 3)
                sq = (1, 7)[(i + j) % 2]
                scale = SMX_SCALES[(i // 2 + j) % 2]
                name = f"smx/{DT_NAME[dt]}-{mode}-sk{sk}-sq{sq}"
                out[name] = SmxCase(name, dt, b, h, sq, sk, f32(scale), mode)
        # full blocks only: 2 * 2 * 1 rows, and 2 * 2 * 7
        for mode, sq, sk in (("none", 1, 512), ("maskh", 7, 1032)):
            name = f"smx/{DT_NAME[dt]}-{mode}-sk{sk}-sq{sq}-rows4k"
            out[name] = SmxCase(name, dt, 2, 2, sq, sk, f32(0.125), mode)
        name = f"smx/{DT_NAME[dt]}-none-sk520-sq7-neginf"
        out[name] = SmxCase(name, dt, 1, 3, 7, 520, f32(1.0), "none", neginf=True)
    return out


SMX_CASES = _smx_cases()


def smx_inputs(case: SmxCase):
    """(x, dy, mask or None) on the CPU. x = randn * 4; "maskh" masks its last row completely (the
    kernel then gives the uniform 1 / sk); a neginf case has -inf inputs, among them a whole
    16-byte pack and the row maximum's neighbours."""
    g = _gen(case.name)
    shape = (case.b, case.h, case.sq, case.sk)
    x = (torch.randn(shape, generator=g) * 4).to(case.dtype)
    dy = torch.randn(shape, generator=g).to(case.dtype)
    mask = None
    if case.mode in ("mask1", "maskh"):
        mh = 1 if case.mode == "mask1" else case.h
        mask = (torch.rand((case.b, mh, case.sq, case.sk), generator=g) < 0.3).to(torch.uint8)
        if case.mode == "maskh":
            mask[-1, -1, -1, :] = 1
    if case.neginf:
        x[..., 0, 8:16] = -INF
        x[..., 1, ::3] = -INF
        x[0, 0, 2, 1:] = -INF
    return x, dy, mask


# ----------------------------------------------------------------------------
# cross-entropy cases
# ----------------------------------------------------------------------------
XENT_N = 7
# 2: BERT's NSP head; 2048 / 2056: one sweep of the 256 x 8 block and the first column of the second
XENT_V = [2, 8, 1000, 2048, 2056, 50257, 50304]
XENT_SMOOTHING = [0.0, 0.1]
XENT_IGNORE = [0, -1, -100]
XENT_PAD_FROM = 50257   # the -inf case: columns >= this are masked to -inf


@dataclass(frozen=True)
class XentCase:
    name: str
    dtype: torch.dtype
    V: int
    smoothing: float
    ignore_index: int
    kind: str = "plain"    # "plain" | "neginf" | "shift" (x + 1000) | "big" (fp16 logits near +-60000)
    seed: str = ""         # cases with the same seed share their random draws (default: the name)


def _xent_cases():
    out = {}
    for a, dt in enumerate(DTYPES):
        for i, V in enumerate(XENT_V):
            for j, s in enumerate(XENT_SMOOTHING):
                ign = XENT_IGNORE[(a + i + j) % 3]
                name = f"xent/{DT_NAME[dt]}-V{V}-s{s}-ign{ign}"
                out[name] = XentCase(name, dt, V, f32(s), ign)
        name = f"xent/{DT_NAME[dt]}-V50304-s0.0-ign-100-neginf"
        out[name] = XentCase(name, dt, 50304, 0.0, -100, "neginf")
    # shift invariance: the same draws as they are and moved by 1000
    for V in (1000, 2056):
        for s in XENT_SMOOTHING:
            for kind in ("plain", "shift"):
                name = f"xent/f32-V{V}-s{s}-ign-100-pair-{kind}"
                out[name] = XentCase(name, F32, V, f32(s), -100, kind, seed=f"xent-pair-V{V}-s{s}")
    out["xent/f16-V2056-s0.1-ign-100-big"] = XentCase("xent/f16-V2056-s0.1-ign-100-big", F16, 2056, f32(0.1), -100,
                                                      "big")
    return out


XENT_CASES = _xent_cases()


def xent_inputs(case: XentCase):
    """(logits [N, V], labels [N], dloss [N] fp32). Row 2 is labelled ignore_index, row 4 has a label
    >= V, row 5 a negative label that is not ignore_index."""
    g = _gen(case.seed or case.name)
    N, V = XENT_N, case.V
    xf = torch.randn((N, V), generator=g) * 3
    labels = torch.randint(0, V, (N,), generator=g)
    dloss = torch.rand((N,), generator=g) + 0.5
    if case.kind == "shift":
        xf = xf + 1000.0
    if case.kind == "big":
        xf = torch.where(torch.rand((N, V), generator=g) < 0.5, 60000.0 + xf, -60000.0 + xf)
    x = xf.to(case.dtype)
    if case.kind == "neginf":
        x[:, XENT_PAD_FROM:] = -INF
        labels = labels.clamp(max=XENT_PAD_FROM - 1)
    labels[2] = case.ignore_index
    labels[4] = V + 3
    labels[5] = -7 if case.ignore_index != -7 else -8
    return x, labels, dloss


# ----------------------------------------------------------------------------
# LayerNorm / RMSNorm cases
# ----------------------------------------------------------------------------
# fast path VPT 1 (8 .. 512), 2 (520, 1024), 4 (1032, 2048; backward), forward VPT 8 and wide
# backward VPT 5 .. 8 (2056, 2560, 4096), slow path (100: cols % 8 != 0, 5000: > 4096)
LN_COLS = [8, 64, 504, 512, 520, 1024, 1032, 2048, 2056, 2560, 4096, 100, 5000]
LN_PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (BF16, F32), (F16, F32)]   # (activation, weight)
LN_EPS = 1e-5


@dataclass(frozen=True)
class NormCase:
    name: str
    xdt: torch.dtype
    wdt: torch.dtype
    rows: int
    cols: int
    rms: bool
    affine: bool = True
    shift: float = 0.0
    stats: str = ""        # BOUNDS key: mean / rstd depend on x alone

    @property
    def eps(self):
        return f32(LN_EPS)


def _norm_case(xdt, wdt, rows, cols, rms, affine=True, shift=0.0, tag=""):
    kind = "rms" if rms else "ln"
    stats = f"{kind}/{DT_NAME[xdt]}-r{rows}-c{cols}" + (f"-shift{shift:g}" if shift else "")
    name = f"{kind}/{DT_NAME[xdt]}-w{DT_NAME[wdt] if affine else 'none'}-r{rows}-c{cols}" + \
        (f"-shift{shift:g}" if shift else "") + tag
    return NormCase(name, xdt, wdt, rows, cols, rms, affine, shift, stats)


def _norm_cases():
    out = {}
    for i, cols in enumerate(LN_COLS):
        for j, (xdt, wdt) in enumerate(LN_PAIRS):
            for rms in (False, True):
                c = _norm_case(xdt, wdt, (1, 5)[(i + j) % 2], cols, rms)
                out[c.name] = c
    # no affine parameters on the fast, wide and slow paths
    for cols in (512, 1032, 2560, 100):
        for dt in DTYPES:
            for rms in (False, True):
                c = _norm_case(dt, dt, 5, cols, rms, affine=False)
                out[c.name] = c
    # a wave owns two rows and the last block is ragged (3077 = 384 * 8 + 5)
    for xdt, wdt, rms in ((BF16, BF16, False), (F32, F32, True), (F16, F32, False)):
        c = _norm_case(xdt, wdt, 3077, 64, rms)
        out[c.name] = c
    for cols in (512, 100):
        for rms in (False, True):
            c = _norm_case(F32, F32, 5, cols, rms, shift=100.0)
            out[c.name] = c
    return out


NORM_CASES = _norm_cases()


def norm_inputs(case: NormCase):
    """(x [rows, cols], gamma, beta, dy) on the CPU; gamma / beta None without affine parameters,
    beta None for RMSNorm. x depends on (kind, activation dtype, rows, cols, shift) alone."""
    g = _gen(case.stats)
    x = (torch.randn((case.rows, case.cols), generator=g) + case.shift).to(case.xdt)
    dy = torch.randn((case.rows, case.cols), generator=g).to(case.xdt)
    gamma = beta = None
    if case.affine:
        gamma = (1.0 + 0.5 * torch.randn((case.cols,), generator=g)).to(case.wdt)
        if not case.rms:
            beta = torch.randn((case.cols,), generator=g).to(case.wdt)
    return x, gamma, beta, dy


@functools.lru_cache(maxsize=None)
def norm_reference(name: str):
    """ref_norm_fwd + ref_norm_bwd of a case, computed once. Treat as read-only."""
    case = NORM_CASES[name]
    x, gamma, beta, dy = norm_inputs(case)
    fwd = ref_norm_fwd(x, gamma, beta, case.eps, case.rms)
    return {**fwd, **ref_norm_bwd(dy, fwd, case.rms)}


# ----------------------------------------------------------------------------
# Measured bounds of the fp32-valued per-row scalars: largest |fp32 CPU formulation - float64
# reference| over the rows of each case. Cross-entropy: (lse, loss) of softmax_xentropy on CPU
# tensors and torch.logsumexp. Norms: (mean, rstd) of x.float().mean / rsqrt(var + eps), what
# F.layer_norm and _ref_rms compute. Each entry is the measured figure rounded up in its third
# digit; tests/test_row_reference.py measures again and asserts measured <= bound <= 1.02 * measured
# (bound 0 exactly when the fp32 result is exact). The GPU tests allow MARGIN x these plus
# SCALAR_FAST * max(1, |ref|).
# ----------------------------------------------------------------------------
BOUNDS = {
    "xent/f32-V2-s0.0-ign0": (2.15e-07, 4.13e-07),   # measured 2.1459e-07, 4.1208e-07
    "xent/f32-V2-s0.1-ign-1": (1.34e-07, 1.56e-07),   # measured 1.3334e-07, 1.5544e-07
    "xent/f32-V8-s0.0-ign-1": (2.30e-07, 2.98e-07),   # measured 2.2908e-07, 2.9720e-07
    "xent/f32-V8-s0.1-ign-100": (1.95e-07, 1.16e-07),   # measured 1.9473e-07, 1.1588e-07
    "xent/f32-V1000-s0.0-ign-100": (4.60e-07, 5.54e-07),   # measured 4.5919e-07, 5.5320e-07
    "xent/f32-V1000-s0.1-ign0": (4.58e-07, 9.73e-07),   # measured 4.5787e-07, 9.7227e-07
    "xent/f32-V2048-s0.0-ign0": (5.66e-07, 3.79e-07),   # measured 5.6544e-07, 3.7861e-07
    "xent/f32-V2048-s0.1-ign-1": (6.69e-07, 1.63e-06),   # measured 6.6845e-07, 1.6294e-06
    "xent/f32-V2056-s0.0-ign-1": (5.19e-07, 5.19e-07),   # measured 5.1843e-07, 5.1843e-07
    "xent/f32-V2056-s0.1-ign-100": (3.19e-07, 9.27e-07),   # measured 3.1858e-07, 9.2636e-07
    "xent/f32-V50257-s0.0-ign-100": (5.70e-07, 1.28e-06),   # measured 5.6954e-07, 1.2714e-06
    "xent/f32-V50257-s0.1-ign0": (6.87e-07, 8.41e-07),   # measured 6.8601e-07, 8.4033e-07
    "xent/f32-V50304-s0.0-ign0": (3.58e-07, 2.62e-06),   # measured 3.5762e-07, 2.6112e-06
    "xent/f32-V50304-s0.1-ign-1": (5.24e-07, 5.61e-07),   # measured 5.2306e-07, 5.6034e-07
    "xent/f32-V50304-s0.0-ign-100-neginf": (4.93e-07, 1.46e-06),   # measured 4.9283e-07, 1.4502e-06
    "xent/f16-V2-s0.0-ign-1": (7.93e-08, 3.90e-08),   # measured 7.9241e-08, 3.8911e-08
    "xent/f16-V2-s0.1-ign-100": (2.10e-07, 1.07e-07),   # measured 2.0974e-07, 1.0606e-07
    "xent/f16-V8-s0.0-ign-100": (1.98e-07, 3.60e-07),   # measured 1.9796e-07, 3.5942e-07
    "xent/f16-V8-s0.1-ign0": (1.97e-07, 4.43e-07),   # measured 1.9609e-07, 4.4283e-07
    "xent/f16-V1000-s0.0-ign0": (4.08e-07, 3.96e-07),   # measured 4.0787e-07, 3.9516e-07
    "xent/f16-V1000-s0.1-ign-1": (4.95e-07, 5.57e-07),   # measured 4.9433e-07, 5.5658e-07
    "xent/f16-V2048-s0.0-ign-1": (4.67e-07, 2.80e-07),   # measured 4.6644e-07, 2.7944e-07
    "xent/f16-V2048-s0.1-ign-100": (5.55e-07, 7.16e-07),   # measured 5.5488e-07, 7.1546e-07
    "xent/f16-V2056-s0.0-ign-100": (5.17e-07, 5.33e-07),   # measured 5.1691e-07, 5.3254e-07
    "xent/f16-V2056-s0.1-ign0": (5.35e-07, 1.06e-06),   # measured 5.3462e-07, 1.0522e-06
    "xent/f16-V50257-s0.0-ign0": (5.48e-07, 1.37e-06),   # measured 5.4714e-07, 1.3602e-06
    "xent/f16-V50257-s0.1-ign-1": (4.65e-07, 6.26e-07),   # measured 4.6465e-07, 6.2578e-07
    "xent/f16-V50304-s0.0-ign-1": (4.39e-07, 1.74e-06),   # measured 4.3860e-07, 1.7361e-06
    "xent/f16-V50304-s0.1-ign-100": (4.82e-07, 1.13e-06),   # measured 4.8159e-07, 1.1298e-06
    "xent/f16-V50304-s0.0-ign-100-neginf": (5.14e-07, 1.41e-06),   # measured 5.1310e-07, 1.4031e-06
    "xent/bf16-V2-s0.0-ign-100": (6.74e-08, 4.92e-08),   # measured 6.7323e-08, 4.9150e-08
    "xent/bf16-V2-s0.1-ign0": (1.51e-07, 8.62e-08),   # measured 1.5087e-07, 8.6126e-08
    "xent/bf16-V8-s0.0-ign0": (2.62e-07, 2.64e-07),   # measured 2.6104e-07, 2.6361e-07
    "xent/bf16-V8-s0.1-ign-1": (3.61e-07, 1.23e-06),   # measured 3.6028e-07, 1.2213e-06
    "xent/bf16-V1000-s0.0-ign-1": (4.72e-07, 4.72e-07),   # measured 4.7127e-07, 4.7127e-07
    "xent/bf16-V1000-s0.1-ign-100": (2.78e-07, 7.64e-07),   # measured 2.7729e-07, 7.6386e-07
    "xent/bf16-V2048-s0.0-ign-100": (4.10e-07, 4.10e-07),   # measured 4.0957e-07, 4.0957e-07
    "xent/bf16-V2048-s0.1-ign0": (6.23e-07, 1.36e-06),   # measured 6.2217e-07, 1.3563e-06
    "xent/bf16-V2056-s0.0-ign0": (3.79e-07, 3.79e-07),   # measured 3.7827e-07, 3.7827e-07
    "xent/bf16-V2056-s0.1-ign-1": (5.31e-07, 1.40e-06),   # measured 5.3051e-07, 1.3921e-06
    "xent/bf16-V50257-s0.0-ign-1": (5.27e-07, 1.39e-06),   # measured 5.2611e-07, 1.3812e-06
    "xent/bf16-V50257-s0.1-ign-100": (6.15e-07, 1.01e-06),   # measured 6.1497e-07, 1.0014e-06
    "xent/bf16-V50304-s0.0-ign-100": (5.31e-07, 1.38e-06),   # measured 5.3067e-07, 1.3767e-06
    "xent/bf16-V50304-s0.1-ign0": (4.03e-07, 1.43e-06),   # measured 4.0268e-07, 1.4263e-06
    "xent/bf16-V50304-s0.0-ign-100-neginf": (3.57e-07, 1.21e-06),   # measured 3.5655e-07, 1.2040e-06
    "xent/f32-V1000-s0.0-ign-100-pair-plain": (5.05e-07, 4.17e-07),   # measured 5.0489e-07, 4.1665e-07
    "xent/f32-V1000-s0.0-ign-100-pair-shift": (1.87e-05, 3.56e-07),   # measured 1.8695e-05, 3.5548e-07
    "xent/f32-V1000-s0.1-ign-100-pair-plain": (4.91e-07, 1.07e-06),   # measured 4.9018e-07, 1.0633e-06
    "xent/f32-V1000-s0.1-ign-100-pair-shift": (2.19e-05, 2.64e-05),   # measured 2.1820e-05, 2.6336e-05
    "xent/f32-V2056-s0.0-ign-100-pair-plain": (4.01e-07, 4.47e-07),   # measured 4.0088e-07, 4.4640e-07
    "xent/f32-V2056-s0.0-ign-100-pair-shift": (3.00e-05, 3.54e-07),   # measured 2.9918e-05, 3.5344e-07
    "xent/f32-V2056-s0.1-ign-100-pair-plain": (6.35e-07, 9.52e-07),   # measured 6.3452e-07, 9.5145e-07
    "xent/f32-V2056-s0.1-ign-100-pair-shift": (2.92e-05, 2.31e-05),   # measured 2.9125e-05, 2.3043e-05
    "xent/f16-V2056-s0.1-ign-100-big": (1.93e-03, 2.03e-03),   # measured 1.9262e-03, 2.0224e-03
    "ln/f32-r1-c8": (3.73e-09, 9.88e-09),   # measured 3.7253e-09, 9.8723e-09
    "rms/f32-r1-c8": (0.0, 4.52e-08),   # measured 0.0000e+00, 4.5151e-08
    "ln/f16-r5-c8": (0.0, 6.69e-08),   # measured 0.0000e+00, 6.6837e-08
    "rms/f16-r5-c8": (0.0, 5.60e-08),   # measured 0.0000e+00, 5.5998e-08
    "ln/bf16-r1-c8": (0.0, 1.94e-08),   # measured 0.0000e+00, 1.9364e-08
    "rms/bf16-r1-c8": (0.0, 3.86e-08),   # measured 0.0000e+00, 3.8551e-08
    "ln/bf16-r5-c8": (0.0, 8.56e-08),   # measured 0.0000e+00, 8.5584e-08
    "rms/bf16-r5-c8": (0.0, 3.50e-08),   # measured 0.0000e+00, 3.4994e-08
    "ln/f16-r1-c8": (0.0, 9.40e-08),   # measured 0.0000e+00, 9.3978e-08
    "rms/f16-r1-c8": (0.0, 2.27e-08),   # measured 0.0000e+00, 2.2639e-08
    "ln/f32-r5-c64": (1.96e-08, 9.37e-08),   # measured 1.9529e-08, 9.3632e-08
    "rms/f32-r5-c64": (0.0, 7.21e-08),   # measured 0.0000e+00, 7.2030e-08
    "ln/f16-r1-c64": (0.0, 5.85e-08),   # measured 0.0000e+00, 5.8426e-08
    "rms/f16-r1-c64": (0.0, 8.72e-08),   # measured 0.0000e+00, 8.7113e-08
    "ln/bf16-r5-c64": (0.0, 6.98e-08),   # measured 0.0000e+00, 6.9757e-08
    "rms/bf16-r5-c64": (0.0, 1.30e-07),   # measured 0.0000e+00, 1.2995e-07
    "ln/bf16-r1-c64": (0.0, 1.48e-08),   # measured 0.0000e+00, 1.4757e-08
    "rms/bf16-r1-c64": (0.0, 4.72e-08),   # measured 0.0000e+00, 4.7179e-08
    "ln/f16-r5-c64": (7.46e-09, 7.12e-08),   # measured 7.4506e-09, 7.1134e-08
    "rms/f16-r5-c64": (0.0, 4.06e-08),   # measured 0.0000e+00, 4.0501e-08
    "ln/f32-r1-c504": (6.81e-09, 1.14e-08),   # measured 6.8057e-09, 1.1302e-08
    "rms/f32-r1-c504": (0.0, 2.27e-09),   # measured 0.0000e+00, 2.2639e-09
    "ln/f16-r5-c504": (1.13e-09, 5.52e-08),   # measured 1.1235e-09, 5.5106e-08
    "rms/f16-r5-c504": (0.0, 5.88e-08),   # measured 0.0000e+00, 5.8773e-08
    "ln/bf16-r1-c504": (1.31e-09, 1.83e-08),   # measured 1.3009e-09, 1.8283e-08
    "rms/bf16-r1-c504": (0.0, 1.81e-08),   # measured 0.0000e+00, 1.8054e-08
    "ln/bf16-r5-c504": (1.48e-09, 7.07e-08),   # measured 1.4783e-09, 7.0622e-08
    "rms/bf16-r5-c504": (0.0, 5.30e-08),   # measured 0.0000e+00, 5.2903e-08
    "ln/f16-r1-c504": (6.24e-12, 4.08e-08),   # measured 6.2365e-12, 4.0799e-08
    "rms/f16-r1-c504": (0.0, 4.46e-08),   # measured 0.0000e+00, 4.4576e-08
    "ln/f32-r5-c512": (4.80e-09, 2.00e-08),   # measured 4.7958e-09, 1.9939e-08
    "rms/f32-r5-c512": (0.0, 7.12e-08),   # measured 0.0000e+00, 7.1134e-08
    "ln/f16-r1-c512": (0.0, 1.07e-08),   # measured 0.0000e+00, 1.0678e-08
    "rms/f16-r1-c512": (0.0, 9.22e-09),   # measured 0.0000e+00, 9.2198e-09
    "ln/bf16-r5-c512": (9.32e-10, 5.88e-08),   # measured 9.3132e-10, 5.8768e-08
    "rms/bf16-r5-c512": (0.0, 8.75e-08),   # measured 0.0000e+00, 8.7486e-08
    "ln/bf16-r1-c512": (0.0, 6.96e-08),   # measured 0.0000e+00, 6.9560e-08
    "rms/bf16-r1-c512": (0.0, 6.69e-08),   # measured 0.0000e+00, 6.6833e-08
    "ln/f16-r5-c512": (3.96e-09, 3.65e-08),   # measured 3.9581e-09, 3.6419e-08
    "rms/f16-r5-c512": (0.0, 7.02e-08),   # measured 0.0000e+00, 7.0109e-08
    "ln/f32-r1-c520": (6.28e-09, 3.87e-08),   # measured 6.2760e-09, 3.8649e-08
    "rms/f32-r1-c520": (0.0, 8.57e-08),   # measured 0.0000e+00, 8.5695e-08
    "ln/f16-r5-c520": (1.78e-09, 8.09e-08),   # measured 1.7767e-09, 8.0849e-08
    "rms/f16-r5-c520": (0.0, 5.29e-08),   # measured 0.0000e+00, 5.2833e-08
    "ln/bf16-r1-c520": (9.17e-10, 8.87e-08),   # measured 9.1699e-10, 8.8618e-08
    "rms/bf16-r1-c520": (0.0, 2.65e-09),   # measured 0.0000e+00, 2.6474e-09
    "ln/bf16-r5-c520": (1.61e-09, 4.22e-08),   # measured 1.6047e-09, 4.2182e-08
    "rms/bf16-r5-c520": (0.0, 8.56e-08),   # measured 0.0000e+00, 8.5534e-08
    "ln/f16-r1-c520": (1.21e-09, 4.18e-09),   # measured 1.2036e-09, 4.1740e-09
    "rms/f16-r1-c520": (0.0, 4.05e-08),   # measured 0.0000e+00, 4.0498e-08
    "ln/f32-r5-c1024": (7.05e-09, 5.67e-08),   # measured 7.0472e-09, 5.6691e-08
    "rms/f32-r5-c1024": (0.0, 6.27e-08),   # measured 0.0000e+00, 6.2679e-08
    "ln/f16-r1-c1024": (0.0, 5.74e-08),   # measured 0.0000e+00, 5.7388e-08
    "rms/f16-r1-c1024": (0.0, 2.23e-08),   # measured 0.0000e+00, 2.2282e-08
    "ln/bf16-r5-c1024": (0.0, 4.57e-08),   # measured 0.0000e+00, 4.5618e-08
    "rms/bf16-r5-c1024": (0.0, 4.50e-08),   # measured 0.0000e+00, 4.4910e-08
    "ln/bf16-r1-c1024": (0.0, 1.12e-08),   # measured 0.0000e+00, 1.1139e-08
    "rms/bf16-r1-c1024": (0.0, 7.06e-08),   # measured 0.0000e+00, 7.0556e-08
    "ln/f16-r5-c1024": (3.73e-09, 6.39e-08),   # measured 3.7253e-09, 6.3851e-08
    "rms/f16-r5-c1024": (0.0, 5.32e-08),   # measured 0.0000e+00, 5.3112e-08
    "ln/f32-r1-c1032": (3.83e-09, 1.23e-08),   # measured 3.8207e-09, 1.2211e-08
    "rms/f32-r1-c1032": (0.0, 1.94e-08),   # measured 0.0000e+00, 1.9306e-08
    "ln/f16-r5-c1032": (3.56e-09, 5.63e-08),   # measured 3.5520e-09, 5.6202e-08
    "rms/f16-r5-c1032": (0.0, 7.50e-08),   # measured 0.0000e+00, 7.5000e-08
    "ln/bf16-r1-c1032": (1.68e-09, 4.43e-08),   # measured 1.6749e-09, 4.4223e-08
    "rms/bf16-r1-c1032": (0.0, 2.32e-08),   # measured 0.0000e+00, 2.3143e-08
    "ln/bf16-r5-c1032": (8.96e-10, 5.40e-08),   # measured 8.9522e-10, 5.3971e-08
    "rms/bf16-r5-c1032": (0.0, 6.67e-08),   # measured 0.0000e+00, 6.6680e-08
    "ln/f16-r1-c1032": (1.25e-09, 4.94e-08),   # measured 1.2490e-09, 4.9342e-08
    "rms/f16-r1-c1032": (0.0, 3.85e-09),   # measured 0.0000e+00, 3.8489e-09
    "ln/f32-r5-c2048": (3.88e-09, 5.66e-08),   # measured 3.8744e-09, 5.6533e-08
    "rms/f32-r5-c2048": (0.0, 1.26e-07),   # measured 0.0000e+00, 1.2585e-07
    "ln/f16-r1-c2048": (6.70e-10, 4.49e-08),   # measured 6.6939e-10, 4.4895e-08
    "rms/f16-r1-c2048": (0.0, 6.71e-08),   # measured 0.0000e+00, 6.7032e-08
    "ln/bf16-r5-c2048": (1.40e-09, 4.83e-08),   # measured 1.3970e-09, 4.8214e-08
    "rms/bf16-r5-c2048": (0.0, 7.03e-08),   # measured 0.0000e+00, 7.0229e-08
    "ln/bf16-r1-c2048": (3.50e-10, 1.96e-08),   # measured 3.4925e-10, 1.9569e-08
    "rms/bf16-r1-c2048": (0.0, 5.35e-08),   # measured 0.0000e+00, 5.3402e-08
    "ln/f16-r5-c2048": (5.24e-10, 8.05e-08),   # measured 5.2387e-10, 8.0462e-08
    "rms/f16-r5-c2048": (0.0, 6.34e-08),   # measured 0.0000e+00, 6.3309e-08
    "ln/f32-r1-c2056": (4.62e-09, 2.62e-08),   # measured 4.6167e-09, 2.6145e-08
    "rms/f32-r1-c2056": (0.0, 1.93e-08),   # measured 0.0000e+00, 1.9281e-08
    "ln/f16-r5-c2056": (3.19e-09, 7.28e-08),   # measured 3.1817e-09, 7.2744e-08
    "rms/f16-r5-c2056": (0.0, 6.81e-08),   # measured 0.0000e+00, 6.8047e-08
    "ln/bf16-r1-c2056": (1.26e-10, 2.69e-08),   # measured 1.2502e-10, 2.6871e-08
    "rms/bf16-r1-c2056": (0.0, 3.77e-08),   # measured 0.0000e+00, 3.7681e-08
    "ln/bf16-r5-c2056": (3.64e-09, 3.15e-08),   # measured 3.6383e-09, 3.1493e-08
    "rms/bf16-r5-c2056": (0.0, 1.14e-07),   # measured 0.0000e+00, 1.1309e-07
    "ln/f16-r1-c2056": (6.17e-10, 3.52e-08),   # measured 6.1605e-10, 3.5147e-08
    "rms/f16-r1-c2056": (0.0, 2.43e-08),   # measured 0.0000e+00, 2.4216e-08
    "ln/f32-r5-c2560": (4.34e-09, 9.09e-08),   # measured 4.3339e-09, 9.0893e-08
    "rms/f32-r5-c2560": (0.0, 7.90e-08),   # measured 0.0000e+00, 7.8945e-08
    "ln/f16-r1-c2560": (2.80e-09, 4.67e-08),   # measured 2.7940e-09, 4.6652e-08
    "rms/f16-r1-c2560": (0.0, 7.39e-08),   # measured 0.0000e+00, 7.3875e-08
    "ln/bf16-r5-c2560": (1.31e-09, 5.67e-08),   # measured 1.3039e-09, 5.6609e-08
    "rms/bf16-r5-c2560": (0.0, 8.99e-08),   # measured 0.0000e+00, 8.9868e-08
    "ln/bf16-r1-c2560": (7.46e-10, 2.35e-08),   # measured 7.4506e-10, 2.3419e-08
    "rms/bf16-r1-c2560": (0.0, 8.61e-08),   # measured 0.0000e+00, 8.6005e-08
    "ln/f16-r5-c2560": (2.61e-09, 4.84e-08),   # measured 2.6077e-09, 4.8330e-08
    "rms/f16-r5-c2560": (0.0, 7.16e-08),   # measured 0.0000e+00, 7.1541e-08
    "ln/f32-r1-c4096": (2.11e-10, 2.90e-08),   # measured 2.1064e-10, 2.8950e-08
    "rms/f32-r1-c4096": (0.0, 4.89e-08),   # measured 0.0000e+00, 4.8843e-08
    "ln/f16-r5-c4096": (3.35e-09, 5.19e-08),   # measured 3.3469e-09, 5.1862e-08
    "rms/f16-r5-c4096": (0.0, 7.44e-08),   # measured 0.0000e+00, 7.4373e-08
    "ln/bf16-r1-c4096": (7.57e-10, 4.22e-08),   # measured 7.5670e-10, 4.2156e-08
    "rms/bf16-r1-c4096": (0.0, 4.41e-08),   # measured 0.0000e+00, 4.4024e-08
    "ln/bf16-r5-c4096": (9.32e-10, 4.26e-08),   # measured 9.3132e-10, 4.2570e-08
    "rms/bf16-r5-c4096": (0.0, 5.97e-08),   # measured 0.0000e+00, 5.9636e-08
    "ln/f16-r1-c4096": (1.75e-10, 3.03e-08),   # measured 1.7462e-10, 3.0281e-08
    "rms/f16-r1-c4096": (0.0, 5.91e-08),   # measured 0.0000e+00, 5.9001e-08
    "ln/f32-r5-c100": (2.81e-08, 9.38e-08),   # measured 2.8014e-08, 9.3717e-08
    "rms/f32-r5-c100": (0.0, 5.28e-08),   # measured 0.0000e+00, 5.2766e-08
    "ln/f16-r1-c100": (1.20e-09, 2.49e-08),   # measured 1.1921e-09, 2.4863e-08
    "rms/f16-r1-c100": (0.0, 8.57e-09),   # measured 0.0000e+00, 8.5682e-09
    "ln/bf16-r5-c100": (3.58e-09, 5.21e-08),   # measured 3.5763e-09, 5.2038e-08
    "rms/bf16-r5-c100": (0.0, 3.62e-08),   # measured 0.0000e+00, 3.6179e-08
    "ln/bf16-r1-c100": (3.73e-10, 3.04e-08),   # measured 3.7253e-10, 3.0371e-08
    "rms/bf16-r1-c100": (0.0, 2.45e-08),   # measured 0.0000e+00, 2.4447e-08
    "ln/f16-r5-c100": (3.28e-09, 3.63e-08),   # measured 3.2783e-09, 3.6271e-08
    "rms/f16-r5-c100": (0.0, 5.59e-08),   # measured 0.0000e+00, 5.5825e-08
    "ln/f32-r1-c5000": (1.06e-09, 1.76e-08),   # measured 1.0575e-09, 1.7537e-08
    "rms/f32-r1-c5000": (0.0, 5.79e-09),   # measured 0.0000e+00, 5.7850e-09
    "ln/f16-r5-c5000": (2.50e-09, 3.55e-08),   # measured 2.4945e-09, 3.5495e-08
    "rms/f16-r5-c5000": (0.0, 1.03e-08),   # measured 0.0000e+00, 1.0221e-08
    "ln/bf16-r1-c5000": (2.90e-10, 4.08e-09),   # measured 2.8908e-10, 4.0743e-09
    "rms/bf16-r1-c5000": (0.0, 5.07e-08),   # measured 0.0000e+00, 5.0677e-08
    "ln/bf16-r5-c5000": (1.81e-09, 4.79e-08),   # measured 1.8060e-09, 4.7843e-08
    "rms/bf16-r5-c5000": (0.0, 9.81e-08),   # measured 0.0000e+00, 9.8015e-08
    "ln/f16-r1-c5000": (3.16e-09, 7.11e-08),   # measured 3.1531e-09, 7.1005e-08
    "rms/f16-r1-c5000": (0.0, 5.44e-09),   # measured 0.0000e+00, 5.4359e-09
    "ln/f32-r5-c1032": (4.78e-09, 3.45e-08),   # measured 4.7772e-09, 3.4403e-08
    "rms/f32-r5-c1032": (0.0, 9.32e-08),   # measured 0.0000e+00, 9.3192e-08
    "ln/bf16-r3077-c64": (1.50e-08, 1.17e-07),   # measured 1.4901e-08, 1.1686e-07
    "rms/f32-r3077-c64": (0.0, 1.37e-07),   # measured 0.0000e+00, 1.3670e-07
    "ln/f16-r3077-c64": (1.50e-08, 1.14e-07),   # measured 1.4901e-08, 1.1345e-07
    "ln/f32-r5-c512-shift100": (8.71e-06, 4.49e-08),   # measured 8.7023e-06, 4.4824e-08
    "rms/f32-r5-c512-shift100": (0.0, 5.70e-10),   # measured 0.0000e+00, 5.6919e-10
    "ln/f32-r5-c100-shift100": (4.28e-06, 4.74e-08),   # measured 4.2725e-06, 4.7349e-08
    "rms/f32-r5-c100-shift100": (0.0, 8.04e-10),   # measured 0.0000e+00, 8.0346e-10
}
