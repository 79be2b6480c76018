"""Float64 references of the fused elementwise, residual-LayerNorm and embedding kernels
(csrc/fused_ops.hip: bias_act, bias_dropout_add, colsum, splitk_reduce, the bdaln family, embed_ln_fwd /
embed_ln_bwd, embed_segsum), the error bounds they are held to, and the shared test cases.

A plain helper module in the style of row_reference.py and glu_reference.py: no tests, no fixtures. The
references are written from the formulas in the kernel header comments, in float64, and never call the
extension; inputs enter at their stored (16-bit or fp32) values converted to double.

Dropout keep mask (the comment at the top of csrc/fused_ops.hip and drop_mask8): element e of a launch
keeps iff the 16-bit chunk e & 7 of Philox4x32-7(key = seed, counter = (offset + e // 8, subsequence 0))
is >= thresh; chunk k is the low half of word k >> 1 for even k and the high half for odd k.
thresh = max(1, round(p 65536)) and scale = f32(1 / (1 - thresh / 65536)) (bindings.cpp drop_params), so
the kept fraction and the scale agree exactly. keep_mask evaluates that rule in NumPy with its own Philox
(tests/test_fused_reference.py compares it with attn_reference._philox4x32_7); no reference recovers a
mask from a kernel.

Every output comes with its cond, the sum of the absolute values of the terms its formula adds, and is
held to row_reference.check:  |got - ref| <= HALF_ULP[dtype] |ref| + C cond + TINY[dtype],  C = 2**-16.

    bias_act       a = x + b;  y = act(a),  dx = dy act'(a);  cond_y = cf + |act'| (|x| + |b|),
                   cond_dx = |dy| cf'  (cf, cf' of glu_reference.ref_act; ReLU and identity have no inner
                   sum: cf = 0, cf' = |act'|). ReLU is exact away from 0: the cases keep |a| >= 1/16.
    bias_drop_add  y = res + keep scale (x + b);  cond = |res| + keep scale (|x| + |b|)
                   dx = keep scale dy;  cond = |dx|
    bdaln fwd      s = res + keep scale (x + b) rounded once to the activation dtype, cond as above;
                   y, mean, rstd = LayerNorm of s *as stored* (the kernel normalises to_f(from_f<T>(s))),
                   through row_reference.ref_norm_fwd: the GPU test feeds the s the store_s launch wrote,
                   after that s passed its own check, the way ref_softmax_bwd takes the stored y.
    bdaln bwd      ds = LN_bwd(dy) [+ ds_extra];  dres = ds;  dx = keep scale ds
                   from-output: x-hat = (y - beta) / gamma with y as stored, rstd as stored, and
                   dgamma = sum_rows(dy (y - beta)) / gamma; x-hat's cond is (|y| + |beta|) / |gamma|.
                   That holds the from-output kernel to one rounding of its own formula.
    embedding      s = Ww[id] + Wp[pos] + Wt[type] rounded once; LayerNorm of the stored s; then the mask.
                   backward: dy is masked first; ds, dWp (rows past S zero), dWt, dgamma, dbeta.
    embed_segsum   dW[id] = ascending fp32 sum of the stored ds rows of the run of id in the sorted list.

Column sums (db, dbias, dgamma, dbeta, dWp, dWt) add unrounded fp32 values, so their bound takes
n 2**-24 in place of C, n the number of sequential fp32 additions behind one element, read off the code:

    bias_act / bias_drop_add / colsum:  glu_reference.n_adds(rows)  (col_geom + partial_colsum_kernel)
    bdaln (n_adds_ln):  a wave adds its ln_rows_per_wave(rows) = max(1, ceil(rows / 3072)) rows in sequence
        (rpw adds), the 4 waves of a block combine in LDS (3 adds), and partial_colsum_kernel sums the
        parts = ceil(rows / (4 rpw)) partial rows in 16 groups of ceil(parts / 16) and then the 16 group
        sums in sequence (ceil(parts / 16) + 16 adds):  n = rpw + 3 + ceil(parts / 16) + 16.
    embedding backward: wave w of position pos walks the batch rows b = w, w + nwt, ... (nwt = embed_nwt(B)
        = 16 for B >= 16, else B rounded up to 4): ceil(B / nwt) adds. dWp sums nwt partial rows
        (ceil(nwt / 16) + 16 adds); dgamma / dbeta / dWt sum S nwt partial rows (ceil(S nwt / 16) + 16).
    splitk_reduce: nsplit + 1 terms in sequence, one rounding: (nsplit + 1) 2**-24 sum|terms|.
    embed_segsum:  a run of length L: L 2**-24 sum|ds| plus the one rounding.
The cond of a column sum is the column sum of its summands' conds (glu_reference's docstring says why).
One cond was re-derived for this tighter constant: dgamma of the stored-input backward. row_reference's
cond, sum_rows |dy| rstd (|x| + |mean|), takes the row mean as given; under C = 2**-16 that holds, under
18 x 2**-24 it does not. The mean is itself an fp32 sum of cols terms and carries a few 2**-24 of
mean_j |x_j| of error however small it comes out, x-hat inherits rstd times that, and in a column where
x is near the mean and the mean near 0 the summand dy x-hat has almost no cond to cover it: the fp32 CPU
formulation (F.layer_norm, a correct implementation) is at 4.5 times the bound on
emb/f32-wf32-B4-S1-H520-tv2-equal-p0.25-np4 with the "seedhi" mask (one kept row, x-hat = 2.5e-3). So
dgamma's cond counts the mean by the terms it adds: sum_rows |dy| rstd (|x| + mean_j |x_j|)
(dgamma_cond_sum). The from-output dgamma has no mean in its formula and keeps its cond.

mean / rstd are fp32 scalars per row: BOUNDS holds, per case, the measured error of the fp32 CPU
formulation (s.float().mean, rsqrt(var + eps), what F.layer_norm computes) against this reference, measured
on the CPU by tests/test_fused_reference.py; the GPU tests allow MARGIN times that plus SCALAR_FAST.
"""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass

import numpy as np
import torch

from glu_reference import n_adds, ref_act as _glu_ref_act
from mt_reference import BF16, DT_NAME, F16, F32, HALF_ULP, MARGIN, TINY, f32  # noqa: F401
from row_reference import (C, SCALAR_FAST, WORST, check, ratio, ref_norm_bwd, ref_norm_fwd,  # noqa: F401
                           scalar_excess)

ACT_GELU, ACT_GELU_TANH, ACT_RELU, ACT_NONE, ACT_SILU = 0, 1, 2, 3, 4
ACTS = [ACT_GELU, ACT_GELU_TANH, ACT_RELU, ACT_NONE, ACT_SILU]
ACT_NAME = {ACT_GELU: "geluerf", ACT_GELU_TANH: "gelutanh", ACT_RELU: "relu", ACT_NONE: "id", ACT_SILU: "silu"}
INF = float("inf")
F64 = torch.float64
LN_EPS = f32(1e-5)


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# ----------------------------------------------------------------------------
# dropout keep mask
# ----------------------------------------------------------------------------
def drop_params(p: float):
    """(thresh, scale) as the bindings derive them; thresh 0: no dropout."""
    if p <= 0.0:
        return 0, 1.0
    assert p < 1.0
    th = max(1, int(math.floor(p * 65536.0 + 0.5)))
    return th, (INF if th >= 65536 else f32(1.0 / (1.0 - th / 65536.0)))


def _philox7_words(seed: int, counter: np.ndarray):
    """Philox4x32-7 with key = seed and the 128-bit counter (counter, subsequence 0): [n, 4] uint64 words
    < 2**32. Written from the Random123 round (two 32 x 32 -> 64 multiplies, a permutation, the Weyl key
    schedule), separately from attn_reference's."""
    M = np.uint64(0xFFFFFFFF)
    sh = np.uint64(32)
    ctr = counter.astype(np.uint64)
    x = [ctr & M, ctr >> sh, np.zeros_like(ctr), np.zeros_like(ctr)]
    k = [np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)]
    for _ in range(7):
        prod0 = np.uint64(0xD2511F53) * x[0]      # < 2**64: both factors < 2**32
        prod1 = np.uint64(0xCD9E8D57) * x[2]
        x = [(prod1 >> sh) ^ x[1] ^ k[0], prod1 & M, (prod0 >> sh) ^ x[3] ^ k[1], prod0 & M]
        k = [(k[0] + np.uint64(0x9E3779B9)) & M, (k[1] + np.uint64(0xBB67AE85)) & M]
    return np.stack(x, 1)


def keep_chunks(seed: int, offset: int, n: int) -> np.ndarray:
    """The 16-bit chunk of every element e < n (n % 8 == 0) of a launch, uint64 [n]."""
    assert n % 8 == 0
    e8 = np.arange(n // 8, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = np.uint64(offset & 0xFFFFFFFFFFFFFFFF) + e8     # 64-bit counter, wraps like the kernel's
    w = _philox7_words(seed, ctr)                             # [n / 8, 4]
    lo, hi = w & np.uint64(0xFFFF), w >> np.uint64(16)
    return np.stack([lo, hi], 2).reshape(n)                   # word k >> 1, low half first


def keep_mask(seed: int, offset: int, shape, thresh: int) -> torch.Tensor:
    """bool tensor of `shape`: the keep flag of every element (flat index e) of a launch."""
    n = int(np.prod(shape))
    if thresh == 0:
        return torch.ones(shape, dtype=torch.bool)
    return torch.from_numpy(keep_chunks(seed, offset, n) >= np.uint64(thresh)).reshape(shape)


# counter configurations every dropout case also runs on: a seed with high bits, a low counter word that
# carries inside the tensor (offset + e // 8 passes 2**32 after 2 packs), and an offset above 2**32
CTR_BASE = (11, 3)
CTR_CONFIGS = {"seedhi": (0x9E3779B97F4A7C15 & 0x7FFFFFFFFFFFFFFF, 3), "carry": (11, 2 ** 32 - 2),
               "offhi": (11, 5 * 2 ** 32 + 7)}


# ----------------------------------------------------------------------------
# comparison of column sums
# ----------------------------------------------------------------------------
def colsum_ratio(got, ref, cond, dtype, nadds):
    got = got.detach().cpu().double().reshape(ref.shape)
    assert cond.shape == ref.shape
    if not ref.numel():
        return 0.0, ()
    tol = HALF_ULP[dtype] * ref.abs() + nadds * 2.0 ** -24 * cond + TINY[dtype]
    r = (got - ref).abs() / tol
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, INF))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape))


def check_colsum(got, ref, cond, dtype, nadds, what="", tag=None):
    """|got - ref| <= HALF_ULP |ref| + nadds 2**-24 cond + TINY on every element; returns the worst ratio."""
    worst, idx = colsum_ratio(got, ref, cond, dtype, nadds)
    if tag is not None and worst > WORST.get(tag, (-1.0, ""))[0]:
        WORST[tag] = (worst, what)
    if worst > 1.0:
        g = got.detach().cpu().double().reshape(ref.shape)[idx]
        raise AssertionError(f"{what}: worst |got - ref| / bound = {worst:.4g} at {idx}: got {float(g)!r}, ref "
                             f"{float(ref[idx])!r}, cond {float(cond[idx])!r}, {nadds} adds ({DT_NAME[dtype]})")
    return worst


def n_adds_ln(rows: int) -> int:
    """bdaln backward (module docstring)."""
    rpw = max(1, -(-rows // (4 * 768)))
    parts = -(-rows // (4 * rpw))
    return rpw + 3 + -(-parts // 16) + 16


def embed_nwt(B: int) -> int:
    return 16 if B >= 16 else (B + 3) // 4 * 4


def n_adds_embed(B: int, S: int):
    """(dWp, the S nwt sums dgamma / dbeta / dWt) of the embedding backward (module docstring)."""
    nwt = embed_nwt(B)
    walk = -(-B // nwt)
    return walk + -(-nwt // 16) + 16, walk + -(-(S * nwt) // 16) + 16


# ----------------------------------------------------------------------------
# float64 references
# ----------------------------------------------------------------------------
def ref_act(a, act):
    """(act(a), act'(a), cf, cf') in float64 for the five activations of bias_act."""
    a = a.double()
    if act == ACT_RELU:
        g = (a > 0).double()
        return a.clamp(min=0.0), g, torch.zeros_like(a), g
    if act == ACT_NONE:
        return a, torch.ones_like(a), torch.zeros_like(a), torch.ones_like(a)
    return _glu_ref_act(a, act)


def _bias64(b, cols):
    return b.double().reshape(1, cols) if b is not None else torch.zeros(1, cols, dtype=F64)


def ref_bias_act(x, b, dy, act):
    rows, cols = x.shape
    bd = _bias64(b, cols)
    a = x.double() + bd
    ca = x.double().abs() + bd.abs()
    f, fp, cf, cfp = ref_act(a, act)
    d = dy.double()
    out = {"y": f, "y_cond": cf + fp.abs() * ca, "dx": d * fp, "dx_cond": d.abs() * cfp}
    out["db"] = out["dx"].sum(0)
    out["db_cond"] = out["dx_cond"].sum(0)
    return out


def ref_bda(x, b, res, dy, keep, scale):
    """bias_dropout_add; keep bool [rows, cols] from keep_mask, scale from drop_params (inf: nothing kept)."""
    rows, cols = x.shape
    bd = _bias64(b, cols)
    zero = torch.zeros((rows, cols), dtype=F64)
    sc = 0.0 if scale == INF else float(scale)   # scale = inf goes with an all-false mask
    t = torch.where(keep, sc * (x.double() + bd), zero)
    tc = torch.where(keep, sc * (x.double().abs() + bd.abs()), zero)
    dx = torch.where(keep, sc * dy.double(), zero)
    return {"y": res.double() + t, "y_cond": res.double().abs() + tc, "dx": dx, "dx_cond": dx.abs(),
            "db": dx.sum(0), "db_cond": dx.abs().sum(0)}


def ref_splitk(slabs, out0=None):
    """slabs fp32 [nsplit, n]; out0: the pre-filled fp32 out of accumulate. -> (sum, cond, nterms)."""
    s = slabs.double()
    tot, cond = s.sum(0), s.abs().sum(0)
    if out0 is not None:
        tot, cond = tot + out0.double(), cond + out0.double().abs()
    return tot, cond, slabs.shape[0] + 1


def check_splitk(got, ref, cond, dtype, nterms, what="", tag=None):
    return check_colsum(got, ref, cond, dtype, nterms, what, tag)


def dgamma_cond_sum(dy, s_stored, fwd):
    """dgamma's cond under the column-sum bound (module docstring): x-hat = rstd (x - sum_j x_j / cols) counted
    by every term it adds, sum_rows |dy| rstd (|x| + mean_j |x_j|)."""
    x = s_stored.double().reshape(fwd["xhat"].shape)
    return (dy.double().reshape(x.shape).abs() * fwd["rstd"][:, None] * (x.abs() + x.abs().mean(-1, keepdim=True))).sum(0)


def ref_bdaln_bwd(dy, s_stored, gamma, beta, eps, keep, scale, ds_extra=None, has_bias=True):
    """Backward from the stored LN input. Returns ds (= dres), dx, dgamma, dbeta, dbias with conds."""
    fwd = ref_norm_fwd(s_stored, gamma, beta, eps, False)
    bwd = ref_norm_bwd(dy, fwd, False)
    bwd["dgamma_cond"] = dgamma_cond_sum(dy, s_stored, fwd)
    return _bdaln_tail(bwd["dx"], bwd["dx_cond"], bwd, keep, scale, ds_extra, has_bias)


def _bdaln_tail(ds, ds_cond, sums, keep, scale, ds_extra, has_bias):
    if ds_extra is not None:
        ds = ds + ds_extra.double()
        ds_cond = ds_cond + ds_extra.double().abs()
    sc = 0.0 if scale == INF else float(scale)
    zero = torch.zeros_like(ds)
    dx = torch.where(keep, sc * ds, zero)
    dxc = torch.where(keep, sc * ds_cond, zero)
    out = {"dres": ds, "dres_cond": ds_cond, "dx": dx, "dx_cond": dxc,
           "dgamma": sums["dgamma"], "dgamma_cond": sums["dgamma_cond"],
           "dbeta": sums["dbeta"], "dbeta_cond": sums["dbeta_cond"]}
    if has_bias:
        out["dbias"] = dx.sum(0)
        out["dbias_cond"] = dxc.sum(0)
    return out


def ref_bdaln_bwd_fromy(dy, y_stored, gamma, beta, rstd_stored, keep, scale, has_bias=True):
    """The documented from-output formula on the stored inputs: yc = y - beta, x-hat = yc / gamma,
    dgamma = sum_rows(dy yc) / gamma, ds = rstd (dy gamma - s1 - x-hat s2) with s1 = mean(dy gamma),
    s2 = mean(dy yc) (= mean(dy gamma x-hat)). gamma has no zero here (s_alt covers that)."""
    d, y = dy.double(), y_stored.double()
    cols = y.shape[1]
    g, b = gamma.double().reshape(1, cols), beta.double().reshape(1, cols)
    rs = rstd_stored.double().reshape(-1, 1)
    yc = y - b
    ycc = y.abs() + b.abs()
    xh, xhc = yc / g, ycc / g.abs()
    dyg = d * g
    s1 = dyg.mean(-1, keepdim=True)
    s2 = (d * yc).mean(-1, keepdim=True)
    ds = rs * (dyg - s1 - xh * s2)
    ds_cond = rs * (dyg.abs() + dyg.abs().mean(-1, keepdim=True) + xhc * (d.abs() * ycc).mean(-1, keepdim=True))
    sums = {"dgamma": (d * yc).sum(0) / g[0], "dgamma_cond": (d.abs() * ycc).sum(0) / g[0].abs(),
            "dbeta": d.sum(0), "dbeta_cond": d.abs().sum(0)}
    return _bdaln_tail(ds, ds_cond, sums, keep, scale, None, has_bias)


def ref_embed_sum(ids, tids, Ww, Wp, Wt):
    """s = Ww[id] + Wp[pos] + Wt[type] in float64 [B, S, H] with its cond; tids None: type row 0."""
    B, S = ids.shape
    w = Ww.double()[ids.long()]
    p = Wp.double()[:S][None].expand(B, S, -1)
    t = Wt.double()[tids.long()] if tids is not None else Wt.double()[0][None, None].expand(B, S, -1)
    return w + p + t, w.abs() + p.abs() + t.abs()


def ref_embed_fwd(s_stored, gamma, beta, eps, keep, scale):
    """LayerNorm of the stored s [B, S, H], then the mask: y = keep scale LN(s)."""
    B, S, H = s_stored.shape
    fwd = ref_norm_fwd(s_stored.reshape(B * S, H), gamma, beta, eps, False)
    sc = 0.0 if scale == INF else float(scale)
    k2 = keep.reshape(B * S, H)
    zero = torch.zeros_like(fwd["y"])
    fwd["out"] = torch.where(k2, sc * fwd["y"], zero)
    fwd["out_cond"] = torch.where(k2, sc * fwd["y_cond"], zero)
    return fwd


def ref_embed_bwd(dy, fwd, s_stored, tids, tvocab, npos, keep, scale, B, S):
    """dy [B, S, H] is masked first, then the LayerNorm backward from ref_embed_fwd's statistics."""
    H = dy.shape[-1]
    sc = 0.0 if scale == INF else float(scale)
    d = torch.where(keep.reshape(B * S, H), sc * dy.double().reshape(B * S, H), torch.zeros(B * S, H, dtype=F64))
    bwd = ref_norm_bwd(d, fwd, False)
    bwd["dgamma_cond"] = dgamma_cond_sum(d, s_stored, fwd)
    ds, dsc = bwd["dx"].reshape(B, S, H), bwd["dx_cond"].reshape(B, S, H)
    dWp, dWpc = torch.zeros(npos, H, dtype=F64), torch.zeros(npos, H, dtype=F64)
    dWp[:S], dWpc[:S] = ds.sum(0), dsc.sum(0)
    dWt, dWtc = torch.zeros(tvocab, H, dtype=F64), torch.zeros(tvocab, H, dtype=F64)
    t = tids.long() if tids is not None else torch.zeros(B, S, dtype=torch.long)
    for v in range(tvocab):
        m = (t == v)[..., None].double()
        dWt[v], dWtc[v] = (ds * m).sum((0, 1)), (dsc * m).sum((0, 1))
    return {"ds": ds, "ds_cond": dsc, "dWp": dWp, "dWp_cond": dWpc, "dWt": dWt, "dWt_cond": dWtc,
            "dgamma": bwd["dgamma"], "dgamma_cond": bwd["dgamma_cond"], "dbeta": bwd["dbeta"],
            "dbeta_cond": bwd["dbeta_cond"]}


def ref_segsum(ds_stored, ids, vocab):
    """dW [vocab, H] from the stored ds [R, H]: the rows of each id summed in the order of the stable sort
    (ascending token index). Returns (dW, cond = sum|ds|, run length per id [vocab])."""
    R, H = ds_stored.shape
    flat = ids.reshape(-1).long()
    dW, cond = torch.zeros(vocab, H, dtype=F64), torch.zeros(vocab, H, dtype=F64)
    dW.index_add_(0, flat, ds_stored.double())
    cond.index_add_(0, flat, ds_stored.double().abs())
    return dW, cond, torch.bincount(flat, minlength=vocab)


def check_segsum(got, dW, cond, runs, dtype, what="", tag=None):
    """HALF_ULP |ref| + L 2**-24 cond + TINY per row of run length L; rows without a token must be exact zeros."""
    got64 = got.detach().cpu().double()
    assert got64.shape == dW.shape
    assert not bool(got64[runs == 0].any()), f"{what}: a row without a token is not zero"
    tol = HALF_ULP[dtype] * dW.abs() + runs.double()[:, None] * 2.0 ** -24 * cond + TINY[dtype]
    r = (got64 - dW).abs() / tol
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, INF))
    worst = float(r.max()) if r.numel() else 0.0
    if tag is not None and worst > WORST.get(tag, (-1.0, ""))[0]:
        WORST[tag] = (worst, what)
    assert worst <= 1.0, f"{what}: segsum worst |got - ref| / bound = {worst:.4g} ({DT_NAME[dtype]})"
    return worst


# ----------------------------------------------------------------------------
# cases: column-chunk kernels
# ----------------------------------------------------------------------------
COL_COLS = [8, 2040, 2048, 2056, 4104]      # the 256 x 8 block, both sides of its boundary, a third chunk
COL_ROWS = [1, 16, 17, 33]                  # the 16-row floor of col_geom, ragged and full
COL_BIG_ROWS = 8209                         # rpb = 17 and a ragged last row block
COL_PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (BF16, F32), (F16, F32), (None, None)]   # (x, bias)
NOBIAS_X = [F32, F16, BF16]
DROP_P = [0.1, 0.5, 2.0 ** -16, 1.0 - 2.0 ** -16]


@dataclass(frozen=True)
class ColCase:
    name: str
    xdt: torch.dtype
    bdt: object
    rows: int
    cols: int
    act: int = ACT_NONE
    p: float = 0.0
    kind: str = "randn"      # "randn" | "int" (integer-valued: exact results) | "pos" (randn with dy > 0)


def _col_cases():
    act, bda = {}, {}
    for i, cols in enumerate(COL_COLS):
        for j, (xdt, bdt) in enumerate(COL_PAIRS):
            if xdt is None:
                xdt = NOBIAS_X[i % 3]
            rows = COL_ROWS[(i + j) % 4]
            a = ACTS[(i + 2 * j) % 5]
            n = f"act/{ACT_NAME[a]}-{DT_NAME[xdt]}-b{DT_NAME[bdt]}-r{rows}-c{cols}"
            act[n] = ColCase(n, xdt, bdt, rows, cols, a)
            p = ([0.0] + DROP_P)[(i + j) % 5]
            n = f"bda/{DT_NAME[xdt]}-b{DT_NAME[bdt]}-r{rows}-c{cols}-p{p:.6g}"
            bda[n] = ColCase(n, xdt, bdt, rows, cols, p=p)
    # every activation in every activation dtype, with and without a bias, at the smallest shape
    for xdt, bdt in ((F32, F32), (F16, F32), (BF16, BF16), (F16, None)):
        for a in ACTS:
            n = f"act/{ACT_NAME[a]}-{DT_NAME[xdt]}-b{DT_NAME[bdt]}-r17-c8"
            act[n] = ColCase(n, xdt, bdt, 17, 8, a)
    # every p in every activation dtype
    for xdt, bdt in ((F32, F32), (F16, F16), (BF16, F32)):
        for p in DROP_P:
            n = f"bda/{DT_NAME[xdt]}-b{DT_NAME[bdt]}-r17-c2056-p{p:.6g}"
            bda[n] = ColCase(n, xdt, bdt, 17, 2056, p=p)
    # the large row count once per path
    n = f"act/geluerf-bf16-bf32-r{COL_BIG_ROWS}-c8"
    act[n] = ColCase(n, BF16, F32, COL_BIG_ROWS, 8, ACT_GELU)
    n = f"bda/f16-bf16-r{COL_BIG_ROWS}-c8-p0.1"
    bda[n] = ColCase(n, F16, F16, COL_BIG_ROWS, 8, p=0.1)
    # integer-valued inputs, p = 0: bit-exact results
    for xdt, bdt in ((F32, F32), (F16, F16), (BF16, F32)):
        n = f"act/id-{DT_NAME[xdt]}-b{DT_NAME[bdt]}-r33-c2056-int"
        act[n] = ColCase(n, xdt, bdt, 33, 2056, ACT_NONE, kind="int")
        n = f"act/relu-{DT_NAME[xdt]}-b{DT_NAME[bdt]}-r33-c2056-int"
        act[n] = ColCase(n, xdt, bdt, 33, 2056, ACT_RELU, kind="int")
        n = f"bda/{DT_NAME[xdt]}-b{DT_NAME[bdt]}-r33-c2056-p0-int"
        bda[n] = ColCase(n, xdt, bdt, 33, 2056, kind="int")
    # dy > 0: the bias gradient is a sum of same-sign terms, the one output that tells the quantised
    # 1 / (1 - thresh / 65536) from 1 / (1 - p) (6.8e-6 apart at p = 0.1, below C but above n_adds 2**-24)
    n = "bda/f32-bf32-r33-c2056-p0.1-pos"
    bda[n] = ColCase(n, F32, F32, 33, 2056, p=0.1, kind="pos")
    return act, bda


ACT_CASES, BDA_CASES = _col_cases()


def col_inputs(case: ColCase):
    """(x, bias or None, res, dy) on the CPU. randn: x = 4 randn moved away from -bias so that the
    pre-activation a = x + b has |a| >= 1/16 (ReLU's kink), and |x|, |res|, |dy| >= 1/16 so that a dropped
    element shows as an exact zero. int: small integers (every sum and product exact in every dtype)."""
    g = _gen(case.name)
    shape = (case.rows, case.cols)
    if case.kind == "int":
        x = torch.randint(-3, 4, shape, generator=g).float()
        x = torch.where(x == 0, torch.ones_like(x), x)
        bias = torch.randint(-2, 3, (case.cols,), generator=g).float() * 8 if case.bdt is not None else None
        res = torch.randint(-4, 5, shape, generator=g).float()
        dy = torch.randint(1, 4, shape, generator=g).float() * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
        return x.to(case.xdt), (bias.to(case.bdt) if bias is not None else None), res.to(case.xdt), dy.to(case.xdt)
    bias = torch.randn((case.cols,), generator=g).to(case.bdt) if case.bdt is not None else None
    b64 = bias.double() if bias is not None else torch.zeros(case.cols, dtype=F64)
    a = torch.randn(shape, generator=g).double() * 4
    a = torch.where(a.abs() < 0.125, torch.where(a < 0, -0.125, 0.125).double(), a)
    x = (a - b64).to(case.xdt)
    # the rounding of x moves a; the few elements that end up near 0 (or whose x is near 0) get a = 3 or -3
    far = torch.where((3.0 - b64).abs() >= 1.0, 3.0 - b64, -3.0 - b64).expand(shape)
    bad = ((x.double() + b64).abs() < 0.0625) | (x.double().abs() < 0.0625)
    x = torch.where(bad, far.to(case.xdt), x)
    assert bool(((x.double() + b64).abs() >= 0.0625).all()) and bool((x.double().abs() >= 0.0625).all())

    def away(t):
        return torch.where(t.abs() < 0.0625, torch.where(t < 0, -0.0625, 0.0625).to(t.dtype), t)

    res = away(torch.randn(shape, generator=g)).to(case.xdt)
    dy = away(torch.randn(shape, generator=g)).to(case.xdt)
    if case.kind == "pos":
        dy = dy.abs()
    if case.p > 0.9:
        # scale = 65536: x, the bias and dy go down by 2**-6 (a power of two: the same bits) so that what is
        # kept stays inside fp16's range
        x, dy = x * 2.0 ** -6, dy * 2.0 ** -6
        bias = bias * 2.0 ** -6 if bias is not None else None
    return x, bias, res, dy


@functools.lru_cache(maxsize=None)
def act_reference(name: str):
    case = ACT_CASES[name]
    x, b, _, dy = col_inputs(case)
    return ref_bias_act(x, b, dy, case.act)


def bda_reference(case: ColCase, seed, offset):
    """(ref dict, keep mask) of a bias_dropout_add case on one counter configuration."""
    x, b, res, dy = col_inputs(case)
    th, scale = drop_params(case.p)
    keep = keep_mask(seed, offset, x.shape, th)
    return ref_bda(x, b, res, dy, keep, scale), keep


# ----------------------------------------------------------------------------
# cases: splitk_reduce
# ----------------------------------------------------------------------------
SPLITK_N = [4, 8, 20, 2048, 2056]
SPLITK_NSPLIT = [1, 2, 7]


def splitk_inputs(n, nsplit, integer=False):
    g = _gen(f"splitk-{n}-{nsplit}-{int(integer)}")
    if integer:
        return torch.randint(-8, 9, (nsplit, n), generator=g).float(), torch.randint(-8, 9, (n,), generator=g).float()
    return torch.randn((nsplit, n), generator=g) * 3, torch.randn((n,), generator=g)


# ----------------------------------------------------------------------------
# cases: bdaln
# ----------------------------------------------------------------------------
# VPT 1 / 2 / 4 with idle lanes, then the wide rows (VPT 5 and 8)
BDALN_COLS = [8, 504, 512, 520, 1024, 1032, 2048, 2056, 2560, 4096]
BDALN_ROWS = [1, 3, 4, 5]
BDALN_BIG_ROWS = 3077                        # two rows per wave, ragged last block
BDALN_PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (BF16, F32), (F16, F32)]   # (activation, weight)
BDALN_MODES = ["plain", "nobias", "extra"]
BDALN_BAD_COLS = [100, 4104, 5000]


@dataclass(frozen=True)
class LnCase:
    name: str
    xdt: torch.dtype
    wdt: torch.dtype
    rows: int
    cols: int
    mode: str
    p: float

    @property
    def wide(self):
        return self.cols > 2048

    @property
    def eps(self):
        return LN_EPS


def _ln_case(xdt, wdt, rows, cols, mode, p):
    n = f"bdaln/{DT_NAME[xdt]}-w{DT_NAME[wdt]}-r{rows}-c{cols}-{mode}-p{p:g}"
    return LnCase(n, xdt, wdt, rows, cols, mode, p)


def _bdaln_cases():
    out = {}
    for i, cols in enumerate(BDALN_COLS):
        for j, (xdt, wdt) in enumerate(BDALN_PAIRS):
            c = _ln_case(xdt, wdt, BDALN_ROWS[(i + j) % 4], cols, BDALN_MODES[(i + 2 * j) % 3], (0.0, 0.1)[(i + j // 2) % 2])
            out[c.name] = c
    # every mode with and without dropout in every activation dtype, narrow and wide
    for xdt, wdt in ((F32, F32), (F16, F32), (BF16, BF16)):
        for cols in (520, 2056):
            for mode in BDALN_MODES:
                for p in (0.0, 0.1):
                    c = _ln_case(xdt, wdt, 5, cols, mode, p)
                    out[c.name] = c
    for xdt, wdt, cols, mode in ((BF16, F32, 1032, "plain"), (F16, F16, 2560, "extra")):
        c = _ln_case(xdt, wdt, BDALN_BIG_ROWS, cols, mode, 0.1)
        out[c.name] = c
    return out


BDALN_CASES = _bdaln_cases()


def bdaln_inputs(case: LnCase):
    """dict of CPU tensors: x, bias (None for nobias; in the weight dtype, what the bindings accept), res,
    gamma, beta, dy, ds_extra (extra mode). gamma stays away from 0 (|gamma| >= 0.25): from-output divides by it."""
    g = _gen(case.name)
    shape = (case.rows, case.cols)
    x = torch.randn(shape, generator=g).to(case.xdt)
    res = torch.randn(shape, generator=g).to(case.xdt)
    dy = torch.randn(shape, generator=g).to(case.xdt)
    gam = 1.0 + 0.5 * torch.randn((case.cols,), generator=g)
    gam = torch.where(gam.abs() < 0.25, torch.full_like(gam, 0.25), gam).to(case.wdt)
    beta = torch.randn((case.cols,), generator=g).to(case.wdt)
    bias = torch.randn((case.cols,), generator=g).to(case.wdt) if case.mode != "nobias" else None
    dse = torch.randn(shape, generator=g).to(case.xdt) if case.mode == "extra" else None
    return {"x": x, "bias": bias, "res": res, "gamma": gam, "beta": beta, "dy": dy, "ds_extra": dse}


def ref_bdaln_s(inp, keep, scale):
    """(s, cond) before its one rounding."""
    r = ref_bda(inp["x"], inp["bias"], inp["res"], inp["dy"], keep, scale)
    return r["y"], r["y_cond"]


def cpu_bdaln_s(inp, keep, scale):
    """s of the fp32 composition with the Python mask applied by hand, rounded once to the activation dtype."""
    t = inp["x"].float() + (inp["bias"].float() if inp["bias"] is not None else 0.0)
    if scale != 1.0 or not bool(keep.all()):
        t = torch.where(keep, t * (0.0 if scale == INF else scale), torch.zeros_like(t))
    return (inp["res"].float() + t).to(inp["x"].dtype)


# ----------------------------------------------------------------------------
# cases: BERT embeddings
# ----------------------------------------------------------------------------
EMB_H = [8, 520, 1032, 2048]
EMB_B = [1, 3, 4, 5, 17, 35]
EMB_S = [1, 5]
EMB_PAIRS = [(F16, F16), (BF16, BF16), (BF16, F32), (F32, F32)]   # (activation and tables, gamma / beta)
EMB_TYPES = ["tv2", "tv1", "none"]        # type vocabulary 2 with ids, 1 with ids (all 0), no type ids
EMB_IDS = ["equal", "distinct", "last", "straddle"]
EMB_VOCAB = 200


@dataclass(frozen=True)
class EmbCase:
    name: str
    xdt: torch.dtype
    wdt: torch.dtype
    B: int
    S: int
    H: int
    types: str
    ids: str
    p: float
    npos: int

    @property
    def tvocab(self):
        return 1 if self.types == "tv1" else 2

    @property
    def eps(self):
        return LN_EPS


def _emb_cases():
    out = {}
    for i, H in enumerate(EMB_H):
        for j, B in enumerate(EMB_B):
            xdt, wdt = EMB_PAIRS[(i + j) % 4]
            S = EMB_S[(i + j // 2) % 2]
            types = EMB_TYPES[(i + j) % 3]
            ids = EMB_IDS[(2 * i + j) % 4]
            p = (0.0, 0.25)[(i + j // 3) % 2]
            npos = S + (0, 3)[(i + j) % 2]
            n = f"emb/{DT_NAME[xdt]}-w{DT_NAME[wdt]}-B{B}-S{S}-H{H}-{types}-{ids}-p{p:g}-np{npos}"
            out[n] = EmbCase(n, xdt, wdt, B, S, H, types, ids, p, npos)
    return out


EMB_CASES = _emb_cases()


def emb_inputs(case: EmbCase):
    """dict: ids int32 [B, S], tids int32 [B, S] or None, Ww [V, H], Wp [npos, H], Wt [tvocab, H], gamma, beta,
    dy [B, S, H]. Id sets: all equal; all distinct; the last row of the table among them; runs of equal ids
    that straddle the 4-wave blocks of the sorted list (runs of 3 over the sorted order)."""
    g = _gen(case.name)
    B, S, H, V = case.B, case.S, case.H, EMB_VOCAB
    R = B * S
    if case.ids == "equal":
        ids = torch.full((R,), 7)
    elif case.ids == "distinct":
        ids = torch.randperm(V, generator=g)[:R]
    elif case.ids == "last":
        ids = torch.randint(0, V, (R,), generator=g)
        ids[R // 2] = V - 1
    else:
        ids = (torch.arange(R) // 3 * 5 % V)[torch.randperm(R, generator=g)]
    ids = ids.reshape(B, S).to(torch.int32)
    tids = None
    if case.types == "tv2":
        tids = torch.randint(0, 2, (B, S), generator=g).to(torch.int32)
    elif case.types == "tv1":
        tids = torch.zeros((B, S), dtype=torch.int32)
    Ww = torch.randn((V, H), generator=g).to(case.xdt)
    Wp = torch.randn((case.npos, H), generator=g).to(case.xdt)
    Wt = torch.randn((case.tvocab, H), generator=g).to(case.xdt)
    gamma = (1.0 + 0.5 * torch.randn((H,), generator=g)).to(case.wdt)
    beta = torch.randn((H,), generator=g).to(case.wdt)
    dy = torch.randn((B, S, H), generator=g).to(case.xdt)
    return {"ids": ids, "tids": tids, "Ww": Ww, "Wp": Wp, "Wt": Wt, "gamma": gamma, "beta": beta, "dy": dy}


def cpu_embed_s(inp):
    """s [B, S, H] of the fp32 gather-sum, rounded once to the table dtype."""
    B, S = inp["ids"].shape
    t = inp["Wt"].float()[inp["tids"].long()] if inp["tids"] is not None else inp["Wt"].float()[0]
    return (inp["Ww"].float()[inp["ids"].long()] + inp["Wp"].float()[:S][None] + t).to(inp["Ww"].dtype)


# ----------------------------------------------------------------------------
# whole-op checks shared by the CPU and the GPU tier
# ----------------------------------------------------------------------------
def check_bdaln(case, inp, got, keep, scale, tagbase=None, stats_bound=None):
    """Every output of a bdaln forward + stored-input backward against the float64 reference. got["s"] is checked
    first and then taken as the LayerNorm's input. Returns the ratios."""
    tag = (lambda o, dt: None) if tagbase is None else (lambda o, dt: f"{tagbase}/{o}/{DT_NAME[dt]}")
    n = case.name
    s_ref, s_cond = ref_bdaln_s(inp, keep, scale)
    out = {"s": check(got["s"], s_ref, s_cond, case.xdt, n + " s", tag("s", case.xdt))}
    s_stored = got["s"].detach().cpu()
    fwd = ref_norm_fwd(s_stored, inp["gamma"], inp["beta"], case.eps, False)
    out["y"] = check(got["y"], fwd["y"], fwd["y_cond"], case.xdt, n + " y", tag("y", case.xdt))
    if stats_bound is not None:
        for k, b in zip(("mean", "rstd"), stats_bound):
            out[k] = scalar_excess(got[k].cpu(), fwd[k], b)
            assert out[k] <= 1.0, (n, k, out[k])
    if "dres" in got:
        bwd = ref_bdaln_bwd(inp["dy"], s_stored, inp["gamma"], inp["beta"], case.eps, keep, scale, inp["ds_extra"],
                              inp["bias"] is not None)
        out.update(check_bdaln_bwd(case, got, bwd, tag))
    return out


def check_bdaln_bwd(case, got, bwd, tag=lambda o, dt: None, prefix=""):
    n, na = case.name, n_adds_ln(case.rows)
    out = {}
    for k in ("dres", "dx"):
        if got.get(k) is not None:
            out[k] = check(got[k], bwd[k], bwd[k + "_cond"], case.xdt, f"{n} {prefix}{k}", tag(prefix + k, case.xdt))
    for k in ("dgamma", "dbeta", "dbias"):
        if k in bwd:
            out[k] = check_colsum(got[k], bwd[k], bwd[k + "_cond"], case.wdt, na, f"{n} {prefix}{k}",
                                    tag(prefix + k, case.wdt))
        else:
            assert got.get(k) is None or got[k].numel() == 0
    return out


def check_embed(case, inp, got, keep, scale, tagbase=None, stats_bound=None):
    tag = (lambda o, dt: None) if tagbase is None else (lambda o, dt: f"{tagbase}/{o}/{DT_NAME[dt]}")
    n, B, S, H = case.name, case.B, case.S, case.H
    s_ref, s_cond = ref_embed_sum(inp["ids"], inp["tids"], inp["Ww"], inp["Wp"], inp["Wt"])
    out = {"s": check(got["s"], s_ref, s_cond, case.xdt, n + " s", tag("s", case.xdt))}
    s_stored = got["s"].detach().cpu()
    fwd = ref_embed_fwd(s_stored, inp["gamma"], inp["beta"], case.eps, keep, scale)
    out["y"] = check(got["y"].reshape(B * S, H), fwd["out"], fwd["out_cond"], case.xdt, n + " y", tag("y", case.xdt))
    if stats_bound is not None:
        for k, b in zip(("mean", "rstd"), stats_bound):
            out[k] = scalar_excess(got[k].cpu().reshape(-1), fwd[k], b)
            assert out[k] <= 1.0, (n, k, out[k])
    bwd = ref_embed_bwd(inp["dy"], fwd, s_stored, inp["tids"], case.tvocab, case.npos, keep, scale, B, S)
    out["ds"] = check(got["ds"], bwd["ds"], bwd["ds_cond"], case.xdt, n + " ds", tag("ds", case.xdt))
    n_pos, n_tg = n_adds_embed(B, S)
    for k, dt, na in (("dWp", case.xdt, n_pos), ("dWt", case.xdt, n_tg), ("dgamma", case.wdt, n_tg),
                      ("dbeta", case.wdt, n_tg)):
        out[k] = check_colsum(got[k], bwd[k], bwd[k + "_cond"], dt, na, f"{n} {k}", tag(k, dt))
    assert not bool(got["dWp"].detach().cpu()[S:].any()), "position rows past S must be zero"
    ds_stored = got["ds"].detach().cpu().reshape(B * S, H)
    dW, cond, runs = ref_segsum(ds_stored, inp["ids"], EMB_VOCAB)
    out["dWw"] = check_segsum(got["dWw"], dW, cond, runs, case.xdt, n + " dWw", tag("dWw", case.xdt))
    return out


# ----------------------------------------------------------------------------
# Measured bounds of mean / rstd: largest |fp32 CPU formulation - float64 reference| over the rows of each
# case, on the s of the fp32 CPU composition (cpu_bdaln_s with the base counter configuration; the gather-sum
# for the embedding cases). Each entry is the measured figure rounded up in its third digit;
# tests/test_fused_reference.py measures again and asserts measured <= bound <= 1.02 * measured.
# ----------------------------------------------------------------------------
def measure_stats(s_stored, eps):
    """(mean error, rstd error) of x.float().mean / rsqrt(var + eps) against ref_norm_fwd on s [rows, cols]."""
    ref = ref_norm_fwd(s_stored, None, None, eps, False)
    xf = s_stored.float()
    mean = xf.mean(-1)
    rstd = torch.rsqrt(xf.var(-1, unbiased=False) + eps)
    return float((mean.double() - ref["mean"]).abs().max()), float((rstd.double() - ref["rstd"]).abs().max())


def stats_input(name: str):
    """The stored s [rows, cols] and eps that BOUNDS[name] is measured on."""
    if name in BDALN_CASES:
        case = BDALN_CASES[name]
        inp = bdaln_inputs(case)
        th, scale = drop_params(case.p)
        keep = keep_mask(*CTR_BASE, inp["x"].shape, th)
        return cpu_bdaln_s(inp, keep, scale), case.eps
    case = EMB_CASES[name]
    return cpu_embed_s(emb_inputs(case)).reshape(case.B * case.S, case.H), case.eps


BOUNDS = {
    "bdaln/f32-wf32-r1-c8-plain-p0": (3.73e-09, 2.85e-08),   # measured 3.7253e-09, 2.8488e-08
    "bdaln/f16-wf16-r3-c8-extra-p0": (0.0, 5.71e-08),   # measured 0.0000e+00, 5.7082e-08
    "bdaln/bf16-wbf16-r4-c8-nobias-p0.1": (0.0, 8.81e-09),   # measured 0.0000e+00, 8.8001e-09
    "bdaln/bf16-wf32-r5-c8-plain-p0.1": (0.0, 5.33e-08),   # measured 0.0000e+00, 5.3275e-08
    "bdaln/f16-wf32-r1-c8-extra-p0": (0.0, 4.20e-09),   # measured 0.0000e+00, 4.1907e-09
    "bdaln/f32-wf32-r3-c504-nobias-p0.1": (9.43e-09, 2.48e-08),   # measured 9.4241e-09, 2.4761e-08
    "bdaln/f16-wf16-r4-c504-plain-p0.1": (1.42e-09, 2.53e-08),   # measured 1.4192e-09, 2.5218e-08
    "bdaln/bf16-wbf16-r5-c504-extra-p0": (3.32e-09, 2.81e-08),   # measured 3.3114e-09, 2.8054e-08
    "bdaln/bf16-wf32-r1-c504-nobias-p0": (2.96e-10, 9.84e-09),   # measured 2.9566e-10, 9.8302e-09
    "bdaln/f16-wf32-r3-c504-plain-p0.1": (2.02e-09, 3.60e-08),   # measured 2.0105e-09, 3.5979e-08
    "bdaln/f32-wf32-r4-c512-extra-p0": (2.65e-09, 4.75e-08),   # measured 2.6412e-09, 4.7482e-08
    "bdaln/f16-wf16-r5-c512-nobias-p0": (0.0, 2.79e-08),   # measured 0.0000e+00, 2.7879e-08
    "bdaln/bf16-wbf16-r1-c512-plain-p0.1": (0.0, 1.21e-08),   # measured 0.0000e+00, 1.2034e-08
    "bdaln/bf16-wf32-r3-c512-extra-p0.1": (0.0, 2.22e-08),   # measured 0.0000e+00, 2.2175e-08
    "bdaln/f16-wf32-r4-c512-nobias-p0": (0.0, 5.93e-08),   # measured 0.0000e+00, 5.9254e-08
    "bdaln/f32-wf32-r5-c520-plain-p0.1": (1.64e-08, 4.54e-08),   # measured 1.6322e-08, 4.5361e-08
    "bdaln/f16-wf16-r1-c520-extra-p0.1": (1.44e-10, 1.66e-08),   # measured 1.4328e-10, 1.6526e-08
    "bdaln/bf16-wbf16-r3-c520-nobias-p0": (2.64e-09, 2.64e-08),   # measured 2.6364e-09, 2.6333e-08
    "bdaln/bf16-wf32-r4-c520-plain-p0": (7.34e-09, 2.74e-08),   # measured 7.3360e-09, 2.7377e-08
    "bdaln/f16-wf32-r5-c520-extra-p0.1": (1.72e-09, 3.00e-08),   # measured 1.7194e-09, 2.9907e-08
    "bdaln/f32-wf32-r1-c1024-nobias-p0": (1.15e-09, 4.81e-08),   # measured 1.1496e-09, 4.8084e-08
    "bdaln/f16-wf16-r3-c1024-plain-p0": (0.0, 1.12e-08),   # measured 0.0000e+00, 1.1197e-08
    "bdaln/bf16-wbf16-r4-c1024-extra-p0.1": (1.87e-09, 4.69e-08),   # measured 1.8626e-09, 4.6895e-08
    "bdaln/bf16-wf32-r5-c1024-nobias-p0.1": (0.0, 3.51e-08),   # measured 0.0000e+00, 3.5045e-08
    "bdaln/f16-wf32-r1-c1024-plain-p0": (5.59e-09, 2.89e-09),   # measured 5.5879e-09, 2.8849e-09
    "bdaln/f32-wf32-r3-c1032-extra-p0.1": (1.57e-08, 2.86e-08),   # measured 1.5699e-08, 2.8585e-08
    "bdaln/f16-wf16-r4-c1032-nobias-p0.1": (8.61e-09, 2.76e-08),   # measured 8.6057e-09, 2.7598e-08
    "bdaln/bf16-wbf16-r5-c1032-plain-p0": (1.22e-09, 4.43e-08),   # measured 1.2129e-09, 4.4292e-08
    "bdaln/bf16-wf32-r1-c1032-extra-p0": (3.76e-10, 1.51e-08),   # measured 3.7542e-10, 1.5072e-08
    "bdaln/f16-wf32-r3-c1032-nobias-p0.1": (1.28e-09, 3.70e-08),   # measured 1.2706e-09, 3.6946e-08
    "bdaln/f32-wf32-r4-c2048-plain-p0": (4.87e-09, 1.87e-08),   # measured 4.8612e-09, 1.8686e-08
    "bdaln/f16-wf16-r5-c2048-extra-p0": (0.0, 3.99e-08),   # measured 0.0000e+00, 3.9820e-08
    "bdaln/bf16-wbf16-r1-c2048-nobias-p0.1": (0.0, 1.29e-09),   # measured 0.0000e+00, 1.2860e-09
    "bdaln/bf16-wf32-r3-c2048-plain-p0.1": (0.0, 2.81e-08),   # measured 0.0000e+00, 2.8095e-08
    "bdaln/f16-wf32-r4-c2048-extra-p0": (2.04e-09, 2.72e-08),   # measured 2.0373e-09, 2.7182e-08
    "bdaln/f32-wf32-r5-c2056-nobias-p0.1": (4.35e-09, 2.78e-08),   # measured 4.3475e-09, 2.7701e-08
    "bdaln/f16-wf16-r1-c2056-plain-p0.1": (2.32e-09, 1.68e-09),   # measured 2.3192e-09, 1.6766e-09
    "bdaln/bf16-wbf16-r3-c2056-extra-p0": (1.24e-09, 1.72e-08),   # measured 1.2321e-09, 1.7187e-08
    "bdaln/bf16-wf32-r4-c2056-nobias-p0": (3.05e-09, 5.32e-08),   # measured 3.0440e-09, 5.3147e-08
    "bdaln/f16-wf32-r5-c2056-plain-p0.1": (2.77e-09, 4.02e-08),   # measured 2.7650e-09, 4.0167e-08
    "bdaln/f32-wf32-r1-c2560-extra-p0": (3.17e-09, 1.38e-08),   # measured 3.1625e-09, 1.3727e-08
    "bdaln/f16-wf16-r3-c2560-nobias-p0": (1.50e-09, 5.15e-08),   # measured 1.4901e-09, 5.1499e-08
    "bdaln/bf16-wbf16-r4-c2560-plain-p0.1": (2.99e-09, 4.28e-08),   # measured 2.9802e-09, 4.2762e-08
    "bdaln/bf16-wf32-r5-c2560-extra-p0.1": (4.48e-09, 5.78e-08),   # measured 4.4703e-09, 5.7800e-08
    "bdaln/f16-wf32-r1-c2560-nobias-p0": (3.73e-10, 2.53e-08),   # measured 3.7253e-10, 2.5246e-08
    "bdaln/f32-wf32-r3-c4096-plain-p0.1": (3.81e-09, 2.95e-08),   # measured 3.8078e-09, 2.9453e-08
    "bdaln/f16-wf16-r4-c4096-extra-p0.1": (9.32e-10, 4.38e-08),   # measured 9.3132e-10, 4.3736e-08
    "bdaln/bf16-wbf16-r5-c4096-nobias-p0": (0.0, 4.92e-08),   # measured 0.0000e+00, 4.9135e-08
    "bdaln/bf16-wf32-r1-c4096-plain-p0": (0.0, 1.64e-08),   # measured 0.0000e+00, 1.6375e-08
    "bdaln/f16-wf32-r3-c4096-extra-p0.1": (1.63e-09, 2.89e-08),   # measured 1.6298e-09, 2.8888e-08
    "bdaln/f32-wf32-r5-c520-plain-p0": (1.28e-08, 3.66e-08),   # measured 1.2752e-08, 3.6507e-08
    "bdaln/f32-wf32-r5-c520-nobias-p0": (9.45e-09, 6.23e-08),   # measured 9.4493e-09, 6.2283e-08
    "bdaln/f32-wf32-r5-c520-nobias-p0.1": (1.37e-08, 4.58e-08),   # measured 1.3655e-08, 4.5800e-08
    "bdaln/f32-wf32-r5-c520-extra-p0": (2.19e-08, 2.07e-08),   # measured 2.1872e-08, 2.0603e-08
    "bdaln/f32-wf32-r5-c520-extra-p0.1": (1.90e-08, 2.49e-08),   # measured 1.8977e-08, 2.4874e-08
    "bdaln/f32-wf32-r5-c2056-plain-p0": (9.88e-09, 2.30e-08),   # measured 9.8767e-09, 2.2984e-08
    "bdaln/f32-wf32-r5-c2056-plain-p0.1": (8.01e-09, 1.91e-08),   # measured 8.0085e-09, 1.9017e-08
    "bdaln/f32-wf32-r5-c2056-nobias-p0": (2.24e-09, 2.25e-08),   # measured 2.2314e-09, 2.2402e-08
    "bdaln/f32-wf32-r5-c2056-extra-p0": (1.04e-08, 2.41e-08),   # measured 1.0397e-08, 2.4061e-08
    "bdaln/f32-wf32-r5-c2056-extra-p0.1": (1.12e-08, 3.36e-08),   # measured 1.1124e-08, 3.3571e-08
    "bdaln/f16-wf32-r5-c520-plain-p0": (6.88e-10, 4.66e-08),   # measured 6.8775e-10, 4.6501e-08
    "bdaln/f16-wf32-r5-c520-plain-p0.1": (9.17e-10, 3.30e-08),   # measured 9.1699e-10, 3.2998e-08
    "bdaln/f16-wf32-r5-c520-nobias-p0": (2.53e-09, 4.12e-08),   # measured 2.5217e-09, 4.1192e-08
    "bdaln/f16-wf32-r5-c520-nobias-p0.1": (3.56e-09, 4.18e-08),   # measured 3.5534e-09, 4.1734e-08
    "bdaln/f16-wf32-r5-c520-extra-p0": (7.57e-09, 5.14e-08),   # measured 7.5652e-09, 5.1322e-08
    "bdaln/f16-wf32-r5-c2056-plain-p0": (4.08e-09, 4.84e-08),   # measured 4.0732e-09, 4.8350e-08
    "bdaln/f16-wf32-r5-c2056-nobias-p0": (1.77e-09, 2.55e-08),   # measured 1.7684e-09, 2.5486e-08
    "bdaln/f16-wf32-r5-c2056-nobias-p0.1": (3.63e-09, 4.40e-08),   # measured 3.6238e-09, 4.3959e-08
    "bdaln/f16-wf32-r5-c2056-extra-p0": (1.31e-09, 1.66e-08),   # measured 1.3010e-09, 1.6529e-08
    "bdaln/f16-wf32-r5-c2056-extra-p0.1": (3.90e-09, 1.84e-08),   # measured 3.8992e-09, 1.8332e-08
    "bdaln/bf16-wbf16-r5-c520-plain-p0": (3.44e-09, 3.93e-08),   # measured 3.4387e-09, 3.9288e-08
    "bdaln/bf16-wbf16-r5-c520-plain-p0.1": (1.72e-09, 1.95e-08),   # measured 1.7194e-09, 1.9474e-08
    "bdaln/bf16-wbf16-r5-c520-nobias-p0": (9.17e-10, 5.04e-08),   # measured 9.1699e-10, 5.0317e-08
    "bdaln/bf16-wbf16-r5-c520-nobias-p0.1": (3.21e-09, 3.16e-08),   # measured 3.2095e-09, 3.1505e-08
    "bdaln/bf16-wbf16-r5-c520-extra-p0": (1.27e-09, 1.11e-08),   # measured 1.2609e-09, 1.1019e-08
    "bdaln/bf16-wbf16-r5-c520-extra-p0.1": (6.65e-09, 1.58e-08),   # measured 6.6482e-09, 1.5791e-08
    "bdaln/bf16-wbf16-r5-c2056-plain-p0": (1.38e-09, 2.82e-08),   # measured 1.3771e-09, 2.8171e-08
    "bdaln/bf16-wbf16-r5-c2056-plain-p0.1": (3.40e-09, 3.37e-08),   # measured 3.3919e-09, 3.3633e-08
    "bdaln/bf16-wbf16-r5-c2056-nobias-p0": (1.64e-09, 2.83e-08),   # measured 1.6380e-09, 2.8223e-08
    "bdaln/bf16-wbf16-r5-c2056-nobias-p0.1": (1.40e-09, 3.73e-08),   # measured 1.3915e-09, 3.7203e-08
    "bdaln/bf16-wbf16-r5-c2056-extra-p0": (1.64e-09, 4.38e-08),   # measured 1.6380e-09, 4.3742e-08
    "bdaln/bf16-wbf16-r5-c2056-extra-p0.1": (2.21e-09, 1.89e-08),   # measured 2.2033e-09, 1.8813e-08
    "bdaln/bf16-wf32-r3077-c1032-plain-p0.1": (1.46e-08, 5.80e-08),   # measured 1.4555e-08, 5.7931e-08
    "bdaln/f16-wf16-r3077-c2560-extra-p0.1": (1.41e-08, 5.75e-08),   # measured 1.4063e-08, 5.7408e-08
    "emb/f16-wf16-B1-S1-H8-tv2-equal-p0-np1": (0.0, 3.39e-09),   # measured 0.0000e+00, 3.3807e-09
    "emb/bf16-wbf16-B3-S1-H8-tv1-distinct-p0-np4": (0.0, 1.44e-08),   # measured 0.0000e+00, 1.4347e-08
    "emb/bf16-wf32-B4-S5-H8-none-last-p0-np5": (0.0, 5.36e-08),   # measured 0.0000e+00, 5.3592e-08
    "emb/f32-wf32-B5-S5-H8-tv2-straddle-p0.25-np8": (4.85e-08, 5.69e-08),   # measured 4.8429e-08, 5.6828e-08
    "emb/f16-wf16-B17-S1-H8-tv1-equal-p0.25-np1": (0.0, 2.72e-08),   # measured 0.0000e+00, 2.7194e-08
    "emb/bf16-wbf16-B35-S1-H8-none-distinct-p0.25-np4": (0.0, 5.19e-08),   # measured 0.0000e+00, 5.1837e-08
    "emb/bf16-wbf16-B1-S5-H520-tv1-last-p0.25-np8": (1.55e-09, 1.85e-08),   # measured 1.5474e-09, 1.8432e-08
    "emb/bf16-wf32-B3-S5-H520-none-straddle-p0.25-np5": (3.67e-09, 4.21e-08),   # measured 3.6680e-09, 4.2017e-08
    "emb/f32-wf32-B4-S1-H520-tv2-equal-p0.25-np4": (1.93e-08, 1.30e-08),   # measured 1.9271e-08, 1.2913e-08
    "emb/f16-wf16-B5-S1-H520-tv1-distinct-p0-np1": (2.41e-09, 3.38e-08),   # measured 2.4071e-09, 3.3782e-08
    "emb/bf16-wbf16-B17-S5-H520-none-last-p0-np8": (7.34e-09, 5.34e-08),   # measured 7.3360e-09, 5.3357e-08
    "emb/bf16-wf32-B35-S5-H520-tv2-straddle-p0-np5": (7.34e-09, 5.09e-08),   # measured 7.3360e-09, 5.0808e-08
    "emb/bf16-wf32-B1-S1-H1032-none-equal-p0-np1": (1.30e-09, 2.49e-08),   # measured 1.2995e-09, 2.4852e-08
    "emb/f32-wf32-B3-S1-H1032-tv2-distinct-p0-np4": (7.95e-09, 3.36e-08),   # measured 7.9451e-09, 3.3584e-08
    "emb/f16-wf16-B4-S5-H1032-tv1-last-p0-np5": (3.53e-09, 3.76e-08),   # measured 3.5231e-09, 3.7538e-08
    "emb/bf16-wbf16-B5-S5-H1032-none-straddle-p0.25-np8": (3.64e-09, 3.25e-08),   # measured 3.6387e-09, 3.2442e-08
    "emb/bf16-wf32-B17-S1-H1032-tv2-equal-p0.25-np1": (3.61e-10, 3.03e-08),   # measured 3.6098e-10, 3.0255e-08
    "emb/f32-wf32-B35-S1-H1032-tv1-distinct-p0.25-np4": (2.08e-08, 3.82e-08),   # measured 2.0800e-08, 3.8199e-08
    "emb/f32-wf32-B1-S5-H2048-tv2-last-p0.25-np8": (7.91e-09, 2.20e-08),   # measured 7.9081e-09, 2.1949e-08
    "emb/f16-wf16-B3-S5-H2048-tv1-straddle-p0.25-np5": (3.73e-09, 4.92e-08),   # measured 3.7253e-09, 4.9176e-08
    "emb/bf16-wbf16-B4-S1-H2048-none-equal-p0.25-np4": (0.0, 2.74e-09),   # measured 0.0000e+00, 2.7338e-09
    "emb/bf16-wf32-B5-S1-H2048-tv2-distinct-p0-np1": (0.0, 2.42e-08),   # measured 0.0000e+00, 2.4182e-08
    "emb/f32-wf32-B17-S5-H2048-tv1-last-p0-np8": (8.89e-09, 5.39e-08),   # measured 8.8858e-09, 5.3856e-08
    "emb/f16-wf16-B35-S5-H2048-none-straddle-p0-np5": (3.73e-09, 4.49e-08),   # measured 3.7253e-09, 4.4830e-08
}
