"""Float64 reference of the gated-activation kernels (csrc/fused_ops.hip glu_fwd / glu_bwd), the error
bound they are held to, and the shared test cases.

A plain helper module in the style of row_reference.py: no tests, no fixtures. With x = [g | u]
([rows, 2F]), bias = [b_g | b_u] (or none), a = g + b_g, v = u + b_u:

    y     = act(a) v
    dgate = dy v act'(a)          dup = dy act(a)          dbias = colsum([dgate | dup])

    SiLU:       s = 1 / (1 + exp(-a)),  act = a s,  act' = s (1 + a (1 - s))
    tanh-GELU:  w = k (a + c a^3), t = tanh(w),  act = 0.5 a (1 + t),
                act' = 0.5 (1 + t) + 0.5 a (1 - t^2) k (1 + 3 c a^2)      k = sqrt(2 / pi), c = 0.044715
    erf-GELU:   e = erf(a / sqrt 2), p = exp(-a^2 / 2) / sqrt(2 pi),  act = 0.5 a (1 + e),  act' = 0.5 (1 + e) + a p

The references are written from these formulas in float64 and never call the extension; inputs enter at
their stored (16-bit or fp32) values converted to double.

Every output comes with its `cond`, the sum of the absolute values of the terms its formula adds
(row_reference's docstring says why), and check(got, ref, cond, dtype) is row_reference's:

    |got - ref| <= HALF_ULP[dtype] |ref| + C cond + TINY[dtype],        C = row_reference.C = 2**-16

C's derivation there (a fast exp of an argument up to 88, a handful of fp32 operations, one divide)
covers these formulas for |a| <= 80; the cases stay inside that. The conds:

    ca  = |g| + |b_g|                    cv = |u| + |b_u|
    cf  = |a s| (SiLU),  0.5 |a| (1 + |t|),  0.5 |a| (1 + |e|)
    cf' = s (1 + |a| (1 + s)) (SiLU),
          0.5 (1 + |t|) + 0.5 |a| (1 + t^2) k (1 + 3 c a^2) (tanh-GELU),
          0.5 (1 + |e|) + |a| p (erf-GELU)
    cond_y     = cf cv + |act'| ca |v|        (the second term: a = g + b_g is itself a rounded sum, and
                                               its 2**-24 ca of error reaches y through act')
    cond_dup   = |dy| (cf + |act'| ca)
    cond_dgate = |dy| cv cf'

1 + t, 1 + e and 1 - t^2 are differences the formulas evaluate in fp32: where the activation is
almost 0 (a well below 0) they carry 2**-24 of absolute error however small they come out, which
is why cf and cf' count 1 and |t| (|e|, t^2) separately.

dbias sums the unrounded fp32 dx values over the rows, so its bound takes n_adds 2**-24 in place of
C: n_adds sequential fp32 additions lose at most n_adds 2**-24 of the sum of the absolute values
of what they add. n_adds is read off the reduction order (csrc/fused_ops.hip col_geom, csrc/common.h
partial_colsum_kernel), not measured:
  - a thread adds the rpb = max(16, ceil(rows / 512)) rows of its row block in sequence: rpb adds;
  - the parts = ceil(rows / rpb) partial rows are summed by 16 groups, each over ceil(parts / 16)
    partial rows in sequence, and the 16 group sums in sequence: ceil(parts / 16) + 16 adds.
  n_adds(rows) = rpb + ceil(parts / 16) + 16        (33 for rows <= 256; 64 for rows = 8209).
dbias's cond is the column sum of cond_dgate (cond_dup), not of |dgate| (|dup|): every summand is
itself the value of a formula and arrives with a few 2**-24 of its own cond in error, so the sum
counts the summands' terms, as row_reference's dgamma cond counts the two terms of x-hat. With one
row (n_adds = 33, no second summand) that holds each dx element to 33 x 2**-24 = 2**-19 of its cond,
an eighth of C: the fast exp C allows for is too coarse for that at |a| near 80 (80 log2(e) 2**-24
ln 2 = 2**-18 relative), so the kernels' SiLU takes the accurate expf.
"""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass

import torch

from mt_reference import BF16, DT_NAME, F16, F32, HALF_ULP, TINY, f32  # noqa: F401
from row_reference import C, WORST, check, ratio  # noqa: F401

ACT_GELU, ACT_GELU_TANH, ACT_SILU = 0, 1, 4
ACTS = [ACT_SILU, ACT_GELU_TANH, ACT_GELU]
ACT_NAME = {ACT_SILU: "silu", ACT_GELU_TANH: "gelutanh", ACT_GELU: "geluerf"}
K_TANH = math.sqrt(2.0 / math.pi)
C_TANH = 0.044715
INF = float("inf")


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# ----------------------------------------------------------------------------
# float64 references
# ----------------------------------------------------------------------------
def ref_act(a, act):
    """(act(a), act'(a), cf, cf') in float64."""
    a = a.double()
    if act == ACT_SILU:
        s = torch.sigmoid(a)
        return a * s, s * (1.0 + a * (1.0 - s)), (a * s).abs(), s * (1.0 + a.abs() * (1.0 + s))
    if act == ACT_GELU_TANH:
        t = torch.tanh(K_TANH * (a + C_TANH * a ** 3))
        poly = K_TANH * (1.0 + 3.0 * C_TANH * a * a)
        f = 0.5 * a * (1.0 + t)
        g = 0.5 * (1.0 + t) + 0.5 * a * (1.0 - t * t) * poly
        return f, g, 0.5 * a.abs() * (1.0 + t.abs()), 0.5 * (1.0 + t.abs()) + 0.5 * a.abs() * (1.0 + t * t) * poly
    assert act == ACT_GELU, act
    e = torch.erf(a / math.sqrt(2.0))
    p = torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
    return 0.5 * a * (1.0 + e), 0.5 * (1.0 + e) + a * p, 0.5 * a.abs() * (1.0 + e.abs()), \
        0.5 * (1.0 + e.abs()) + a.abs() * p


def n_adds(rows: int) -> int:
    """Sequential fp32 additions behind one dbias element (module docstring)."""
    rpb = max(16, -(-rows // 512))
    parts = -(-rows // rpb)
    return rpb + -(-parts // 16) + 16


def ref_glu(x, bias, dy, act):
    """x [rows, 2F], bias [2F] or None, dy [rows, F] -> dict of float64 y, dgate, dup, dbias (dbias [2F])
    with their conds (dbias's goes with n_adds 2**-24 in place of C)."""
    F_ = x.shape[-1] // 2
    xd = x.double()
    g, u = xd[..., :F_], xd[..., F_:]
    if bias is not None:
        bg, bu = bias.double()[:F_], bias.double()[F_:]
    else:
        bg = bu = torch.zeros(F_, dtype=torch.float64)
    a, v = g + bg, u + bu
    ca, cv = g.abs() + bg.abs(), u.abs() + bu.abs()
    f, fp, cf, cfp = ref_act(a, act)
    d = dy.double()
    out = {"y": f * v, "y_cond": cf * cv + fp.abs() * ca * v.abs(),
           "dgate": d * v * fp, "dgate_cond": d.abs() * cv * cfp,
           "dup": d * f, "dup_cond": d.abs() * (cf + fp.abs() * ca)}
    dx = torch.cat([out["dgate"], out["dup"]], -1).reshape(-1, 2 * F_)
    dxc = torch.cat([out["dgate_cond"], out["dup_cond"]], -1).reshape(-1, 2 * F_)
    out["dbias"] = dx.sum(0)
    out["dbias_cond"] = dxc.sum(0)
    return out


def dbias_ratio(got, ref, dtype, rows):
    """(worst |got - ref| / bound, index) for dbias: HALF_ULP |ref| + n_adds 2**-24 cond + TINY."""
    got = got.detach().cpu().double()
    assert got.shape == ref["dbias"].shape, (got.shape, ref["dbias"].shape)
    tol = HALF_ULP[dtype] * ref["dbias"].abs() + n_adds(rows) * 2.0 ** -24 * ref["dbias_cond"] + TINY[dtype]
    r = (got - ref["dbias"]).abs() / tol
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, INF))
    i = int(r.argmax())
    return float(r[i]), (i,)


def check_dbias(got, ref, dtype, rows, what="", tag=None):
    worst, idx = dbias_ratio(got, ref, dtype, rows)
    if tag is not None and worst > WORST.get(tag, (-1.0, ""))[0]:
        WORST[tag] = (worst, what)
    if worst > 1.0:
        raise AssertionError(f"{what}: dbias worst |got - ref| / bound = {worst:.4g} at {idx}: got "
                             f"{float(got.detach().cpu().double()[idx])!r}, ref {float(ref['dbias'][idx])!r} "
                             f"({DT_NAME[dtype]})")
    return worst


# ----------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------
# one 256 x 8 block, both sides of its boundary, and a third block
GLU_F = [8, 2040, 2048, 2056, 4104]
# the 16-row floor of col_geom, ragged and full
GLU_ROWS = [1, 16, 17, 33]
# (activation dtype, bias dtype); None: no bias
GLU_PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (BF16, F32), (F16, F32), (F32, None), (F16, None), (BF16, None)]
GLU_GATES = ["randn4", "pm80"]   # randn * 4; uniform in +-80


@dataclass(frozen=True)
class GluCase:
    name: str
    xdt: torch.dtype
    bdt: object
    rows: int
    F: int
    act: int
    gates: str


def _glu_case(xdt, bdt, rows, F_, act, gates):
    name = f"glu/{ACT_NAME[act]}-{DT_NAME[xdt]}-b{DT_NAME[bdt]}-r{rows}-F{F_}-{gates}"
    return GluCase(name, xdt, bdt, rows, F_, act, gates)


def _glu_cases():
    """Rotated the way row_reference._norm_cases does: every F with every dtype pair, the rows, the
    activation and the gate distribution turning with them so that each value of each meets each
    value of the others somewhere."""
    out = {}
    for i, F_ in enumerate(GLU_F):
        for j, (xdt, bdt) in enumerate(GLU_PAIRS):
            c = _glu_case(xdt, bdt, GLU_ROWS[(i + j) % 4], F_, ACTS[(i + 2 * j) % 3], GLU_GATES[(i + j // 2) % 2])
            out[c.name] = c
    # every activation with both gate distributions in every activation dtype, at the smallest shapes
    for xdt, bdt in ((F32, F32), (F16, F32), (BF16, BF16)):
        for act in ACTS:
            for gates in GLU_GATES:
                c = _glu_case(xdt, bdt, 17, 8, act, gates)
                out[c.name] = c
    # more than 512 x 16 rows: rpb = 17 > 16 and the last row block is ragged (8209 = 482 * 17 + 15)
    for xdt, bdt, act in ((BF16, F32, ACT_SILU), (F32, F32, ACT_GELU)):
        c = _glu_case(xdt, bdt, 8209, 8, act, "randn4")
        out[c.name] = c
    return out


GLU_CASES = _glu_cases()


def glu_inputs(case: GluCase):
    """(x [rows, 2F], bias [2F] or None, dy [rows, F]) on the CPU; the up half, dy and the bias are randn."""
    g = _gen(case.name)
    rows, F_ = case.rows, case.F
    if case.gates == "randn4":
        gate = torch.randn((rows, F_), generator=g) * 4
    else:
        gate = (torch.rand((rows, F_), generator=g) * 2 - 1) * 80
    up = torch.randn((rows, F_), generator=g)
    x = torch.cat([gate, up], 1).to(case.xdt)
    dy = torch.randn((rows, F_), generator=g).to(case.xdt)
    bias = torch.randn((2 * F_,), generator=g).to(case.bdt) if case.bdt is not None else None
    if bias is not None and case.gates == "pm80":
        # keep |a| = |g + b_g| <= 80, the range C was derived for
        x[:, :F_] = (x[:, :F_].double().clamp(-76, 76)).to(case.xdt)
    return x, bias, dy


@functools.lru_cache(maxsize=None)
def glu_reference(name: str):
    """ref_glu of a case, computed once. Treat as read-only."""
    case = GLU_CASES[name]
    x, bias, dy = glu_inputs(case)
    return ref_glu(x, bias, dy, case.act)


def check_all(case: GluCase, y, dx, dbias, tagbase=None):
    """y [rows, F], dx [rows, 2F], dbias [2F] or None against the case's reference; returns the ratios."""
    ref = glu_reference(case.name)
    F_ = case.F
    tag = (lambda o, dt: None) if tagbase is None else (lambda o, dt: f"{tagbase}/{o}/{DT_NAME[dt]}")
    out = {"y": check(y, ref["y"], ref["y_cond"], case.xdt, f"{case.name} y", tag("y", case.xdt)),
           "dgate": check(dx[:, :F_], ref["dgate"], ref["dgate_cond"], case.xdt, f"{case.name} dgate",
                          tag("dgate", case.xdt)),
           "dup": check(dx[:, F_:], ref["dup"], ref["dup_cond"], case.xdt, f"{case.name} dup", tag("dup", case.xdt))}
    if case.bdt is not None:
        out["dbias"] = check_dbias(dbias, ref, case.bdt, case.rows, case.name, tag("dbias", case.bdt))
    return out
