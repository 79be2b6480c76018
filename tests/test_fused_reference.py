"""CPU tier of the fused-kernel tests: the package's own fp32 compositions (the CPU fallbacks of
bias_dropout_add, bias_dropout_add_ln, dense_bias_dropout_add_ln and bert_embeddings, _act_ref and
F.layer_norm) against the float64 references of fused_reference.py by their bounds on every table case,
the float64 references against torch.autograd in float64, the Python dropout mask checked four ways, the
measured mean / rstd bounds, and fifteen mutants that the bounds must reject."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fused_reference as R
from apex.ops import fused as fops
from attn_reference import _philox4x32_7
from fused_reference import check_bdaln, check_bdaln_bwd, check_embed  # noqa: F401
from fused_reference import ACT_CASES, BDA_CASES, BDALN_CASES, BF16, EMB_CASES, F16, F32, F64, INF

SEED, OFF = R.CTR_BASE


def _sc(scale):
    return 0.0 if scale == INF else scale


def _to(t, dt):
    return t.detach().to(dt) if t is not None else None


# ----------------------------------------------------------------------------
# fp32 compositions
# ----------------------------------------------------------------------------
def cpu_bias_act(case, act=None):
    x, b, _, dy = R.col_inputs(case)
    xf = x.float().clone().requires_grad_(True)
    bf = b.float().clone().requires_grad_(True) if b is not None else None
    y = fops._act_ref(xf + bf if bf is not None else xf, case.act if act is None else act)
    y.backward(dy.float())
    return _to(y, case.xdt), _to(xf.grad, case.xdt), _to(bf.grad if bf is not None else None, case.bdt)


def cpu_bda(case, keep, scale):
    """bias_dropout_add's CPU fallback in fp32 for p = 0; the same composition with the Python mask for p > 0."""
    x, b, res, dy = R.col_inputs(case)
    xf, rf = x.float().clone().requires_grad_(True), res.float()
    bf = b.float().clone().requires_grad_(True) if b is not None else None
    if case.p == 0.0:
        y = fops.bias_dropout_add(xf, bf, rf, 0.0)
    else:
        t = xf + bf if bf is not None else xf
        y = rf + torch.where(keep, t * _sc(scale), torch.zeros_like(t))
    y.backward(dy.float())
    return _to(y, case.xdt), _to(xf.grad, case.xdt), _to(bf.grad if bf is not None else None, case.bdt)


def cpu_ln(s_stored, gamma, beta, dy, eps, var_unbiased=False):
    """F.layer_norm in fp32 on the stored s with autograd: y, mean, rstd, ds, dgamma, dbeta (fp32)."""
    sf = s_stored.float().clone().requires_grad_(True)
    gf, bf = gamma.float().clone().requires_grad_(True), beta.float().clone().requires_grad_(True)
    if var_unbiased:
        mu = sf.mean(-1, keepdim=True)
        y = (sf - mu) * torch.rsqrt(sf.var(-1, unbiased=True, keepdim=True) + eps) * gf + bf
    else:
        y = F.layer_norm(sf, (sf.shape[-1],), gf, bf, eps)
    y.backward(dy.float())
    xs = sf.detach()
    return {"y": y.detach(), "mean": xs.mean(-1), "rstd": torch.rsqrt(xs.var(-1, unbiased=False) + eps),
            "ds": sf.grad, "dgamma": gf.grad, "dbeta": bf.grad}


def cpu_bdaln(case, keep, scale, mut=None):
    """The stages of bias_dropout_add_ln's fallback in fp32, s rounded once to the activation dtype in between
    (what the kernel stores and normalises). mut: one of the mutants below."""
    inp = R.bdaln_inputs(case)
    if case.p == 0.0:   # the wrapper's own CPU composition
        bf = inp["bias"].float() if inp["bias"] is not None else None
        s32, _ = fops.bias_dropout_add_ln(inp["x"].float(), bf, inp["res"].float(), inp["gamma"].float(),
                                          inp["beta"].float(), 0.0, case.eps)
        s = s32.to(case.xdt)
    else:
        s32 = None
        s = R.cpu_bdaln_s(inp, keep, scale)
    if mut == "ln_unrounded_s":
        t = inp["x"].float() + (inp["bias"].float() if inp["bias"] is not None else 0.0)
        ln_in = inp["res"].float() + torch.where(keep, t * _sc(scale), torch.zeros_like(t))
    else:
        ln_in = s
    ln = cpu_ln(ln_in, inp["gamma"], inp["beta"], inp["dy"], case.eps, var_unbiased=(mut == "unbiased_var"))
    y = ln["y"].to(case.xdt)
    if mut == "y_second_rounding":
        sf = ln_in.float()
        xg = ((sf - ln["mean"][:, None]) * ln["rstd"][:, None] * inp["gamma"].float()).to(case.xdt).float()
        y = (xg + inp["beta"].float()).to(case.xdt)
    ds = ln["ds"]
    dx_in = ds
    if inp["ds_extra"] is not None:
        ds = ds + inp["ds_extra"].float()
        if mut != "extra_not_in_dx":
            dx_in = ds
    dx = torch.where(keep, dx_in * _sc(scale), torch.zeros_like(ds))
    dres = dx if mut == "mask_on_dres" else ds
    dbias = (dx_in if mut == "dbias_before_mask" else dx).sum(0)
    out = {"s": s, "y": y, "mean": ln["mean"], "rstd": ln["rstd"], "dres": dres.to(case.xdt), "dx": dx.to(case.xdt),
           "dgamma": ln["dgamma"].to(case.wdt), "dbeta": ln["dbeta"].to(case.wdt),
           "dbias": dbias.to(case.wdt) if inp["bias"] is not None else None}
    return inp, out


def _ln_mask(case, seed=SEED, off=OFF):
    th, scale = R.drop_params(case.p)
    return R.keep_mask(seed, off, (case.rows, case.cols), th), scale


def cpu_embed(case, keep, scale, mut=None):
    inp = R.emb_inputs(case)
    B, S, H = case.B, case.S, case.H
    s = R.cpu_embed_s(inp)
    sf = s.float().clone().requires_grad_(True)
    gf, bf = inp["gamma"].float().clone().requires_grad_(True), inp["beta"].float().clone().requires_grad_(True)
    ln = F.layer_norm(sf, (H,), gf, bf, case.eps)
    y = torch.where(keep, ln * _sc(scale), torch.zeros_like(ln))
    y.backward(inp["dy"].float())
    ds = sf.grad
    dWp = torch.zeros(case.npos, H)
    dWp[:S] = ds.sum(0)
    dWt = torch.zeros(case.tvocab, H)
    t = inp["tids"].long() if inp["tids"] is not None else torch.zeros(B, S, dtype=torch.long)
    if mut == "type1_into_row0":
        t = torch.zeros_like(t)
    dWt.index_add_(0, t.reshape(-1), ds.reshape(B * S, H))
    ds_st = ds.to(case.xdt)
    dWw = torch.zeros(R.EMB_VOCAB, H)
    flat = inp["ids"].reshape(-1).long()
    rows = ds_st.float().reshape(B * S, H)
    if mut == "segsum_drops_last":
        order = torch.sort(flat, stable=True).indices
        last = order[-1]           # the last element of the last run
        rows = rows.clone()
        rows[last] = 0.0
    dWw.index_add_(0, flat, rows)
    sd = sf.detach().reshape(B * S, H)
    return inp, {"s": s, "y": y.detach().to(case.xdt), "mean": sd.mean(-1),
                 "rstd": torch.rsqrt(sd.var(-1, unbiased=False) + case.eps), "ds": ds_st, "dWp": dWp.to(case.xdt),
                 "dWt": dWt.to(case.xdt), "dgamma": gf.grad.to(case.wdt), "dbeta": bf.grad.to(case.wdt),
                 "dWw": dWw.to(case.xdt)}


def _emb_mask(case, seed=SEED, off=OFF):
    th, scale = R.drop_params(case.p)
    return R.keep_mask(seed, off, (case.B, case.S, case.H), th), scale


# ----------------------------------------------------------------------------
# every correct fp32 formulation is inside the bound on every table case
# ----------------------------------------------------------------------------
def _check_act(case, y, dx, db):
    ref = R.act_reference(case.name)
    R.check(y, ref["y"], ref["y_cond"], case.xdt, case.name + " y")
    R.check(dx, ref["dx"], ref["dx_cond"], case.xdt, case.name + " dx")
    if case.bdt is not None:
        R.check_colsum(db, ref["db"], ref["db_cond"], case.bdt, R.n_adds(case.rows), case.name + " db")


@pytest.mark.parametrize("name", list(ACT_CASES))
def test_bias_act_composition_inside_bound(name):
    case = ACT_CASES[name]
    y, dx, db = cpu_bias_act(case)
    _check_act(case, y, dx, db)
    if case.kind == "int":
        ref = R.act_reference(name)
        assert torch.equal(y.double(), ref["y"]) and torch.equal(dx.double(), ref["dx"])
        assert db is None or torch.equal(db.double(), ref["db"])


def _check_bda(case, ref, y, dx, db):
    R.check(y, ref["y"], ref["y_cond"], case.xdt, case.name + " y")
    R.check(dx, ref["dx"], ref["dx_cond"], case.xdt, case.name + " dx")
    if case.bdt is not None:
        R.check_colsum(db, ref["db"], ref["db_cond"], case.bdt, R.n_adds(case.rows), case.name + " db")


@pytest.mark.parametrize("name", list(BDA_CASES))
def test_bias_dropout_add_composition_inside_bound(name):
    case = BDA_CASES[name]
    ref, keep = R.bda_reference(case, SEED, OFF)
    _, scale = R.drop_params(case.p)
    y, dx, db = cpu_bda(case, keep, scale)
    _check_bda(case, ref, y, dx, db)
    assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(dx.float()).all())
    if case.p > 0:   # dropped elements: y is res, dx an exact zero
        res = R.col_inputs(case)[2]
        assert torch.equal(y[~keep], res[~keep]) and not bool(dx[~keep].any()) and bool((dx[keep] != 0).all())


@pytest.mark.parametrize("name", list(BDALN_CASES))
def test_bdaln_composition_inside_bound(name):
    case = BDALN_CASES[name]
    keep, scale = _ln_mask(case)
    inp, got = cpu_bdaln(case, keep, scale)
    em, er = R.BOUNDS[name]
    check_bdaln(case, inp, got, keep, scale, stats_bound=(em, er))
    if case.wide or case.mode == "extra":
        return
    # from-output: the documented formula in fp32 on the stored y, beta, gamma and rstd
    y, rstd = got["y"], got["rstd"]
    g32, b32, d32 = inp["gamma"].float(), inp["beta"].float(), inp["dy"].float()
    yc = y.float() - b32
    xh = yc / g32
    s1, s2 = (d32 * g32).mean(-1, keepdim=True), (d32 * yc).mean(-1, keepdim=True)
    ds = rstd[:, None] * (d32 * g32 - s1 - xh * s2)
    dx = torch.where(keep, ds * _sc(scale), torch.zeros_like(ds))
    fy = {"dres": ds.to(case.xdt), "dx": dx.to(case.xdt), "dgamma": ((d32 * yc).sum(0) / g32).to(case.wdt),
          "dbeta": d32.sum(0).to(case.wdt), "dbias": dx.sum(0).to(case.wdt) if inp["bias"] is not None else None}
    ref = R.ref_bdaln_bwd_fromy(inp["dy"], y, inp["gamma"], inp["beta"], rstd, keep, scale, inp["bias"] is not None)
    check_bdaln_bwd(case, fy, ref, prefix="fromy ")


def test_bdaln_wrappers_on_cpu_are_the_composition():
    """bias_dropout_add_ln and dense_bias_dropout_add_ln (identity weight) on fp32 CPU tensors with autograd
    against the float64 reference, and a 16-bit bias next to fp32 LayerNorm parameters: the bias gradient comes
    back in the bias's own dtype."""
    case = BDALN_CASES["bdaln/f32-wf32-r5-c520-plain-p0"]
    inp = R.bdaln_inputs(case)
    keep, scale = _ln_mask(case)
    for dense in (False, True):
        leaves = {k: inp[k].clone().requires_grad_(True) for k in ("x", "bias", "res", "gamma", "beta")}
        if dense:
            y = fops.dense_bias_dropout_add_ln(leaves["x"], torch.eye(case.cols), leaves["bias"], leaves["res"],
                                               leaves["gamma"], leaves["beta"], 0.0, case.eps)
            s = (leaves["res"] + leaves["x"] + leaves["bias"]).detach()
        else:
            s, y = fops.bias_dropout_add_ln(leaves["x"], leaves["bias"], leaves["res"], leaves["gamma"], leaves["beta"],
                                            0.0, case.eps)
            s = s.detach()
        y.backward(inp["dy"])
        sd = s.double()
        got = {"s": s, "y": y.detach(), "dres": leaves["res"].grad, "dx": leaves["x"].grad,
               "dgamma": leaves["gamma"].grad, "dbeta": leaves["beta"].grad, "dbias": leaves["bias"].grad,
               "mean": s.mean(-1), "rstd": torch.rsqrt(s.var(-1, unbiased=False) + case.eps)}
        assert sd.shape == (case.rows, case.cols)
        check_bdaln(case, inp, got, keep, scale)
    # mixed precision: bf16 bias, fp32 gamma / beta, bf16 activations
    b16 = inp["bias"].to(BF16).requires_grad_(True)
    x16, r16 = inp["x"].to(BF16), inp["res"].to(BF16)
    s, y = fops.bias_dropout_add_ln(x16, b16, r16, inp["gamma"], inp["beta"], 0.0, case.eps)
    y.float().backward(inp["dy"])
    assert b16.grad.dtype == BF16 and b16.grad.shape == b16.shape
    assert fops._bdaln_bias_ok(b16, inp["gamma"]) and not fops._bdaln_bias_ok(inp["bias"], inp["gamma"].to(BF16))
    assert fops._bdaln_bias(b16, inp["gamma"]).dtype == F32
    assert torch.equal(fops._bdaln_bias(b16, inp["gamma"]), b16.detach().float())
    assert fops._bdaln_dbias(torch.ones(4), b16).dtype == BF16


@pytest.mark.parametrize("name", list(EMB_CASES))
def test_embedding_composition_inside_bound(name):
    case = EMB_CASES[name]
    keep, scale = _emb_mask(case)
    inp, got = cpu_embed(case, keep, scale)
    check_embed(case, inp, got, keep, scale, stats_bound=R.BOUNDS[name])


@pytest.mark.parametrize("cfg", list(R.CTR_CONFIGS))
def test_embedding_composition_on_the_other_counter_configurations(cfg):
    """The case and mask that dgamma's cond was re-derived on (fused_reference's docstring), and two more masks."""
    case = EMB_CASES["emb/f32-wf32-B4-S1-H520-tv2-equal-p0.25-np4"]
    keep, scale = _emb_mask(case, *R.CTR_CONFIGS[cfg])
    inp, got = cpu_embed(case, keep, scale)
    check_embed(case, inp, got, keep, scale, stats_bound=R.BOUNDS[case.name])


def test_bert_embeddings_fallback_inside_bound():
    """The wrapper's CPU composition itself (fp32, p = 0) with autograd, every gradient against the reference."""
    for name, case in EMB_CASES.items():
        if not (case.xdt == F32 and case.p == 0.0):
            continue
        inp = R.emb_inputs(case)
        lv = {k: inp[k].clone().requires_grad_(True) for k in ("Ww", "Wp", "Wt", "gamma", "beta")}
        tids = inp["tids"].long() if inp["tids"] is not None else None
        y = fops.bert_embeddings(inp["ids"].long(), tids, lv["Ww"], lv["Wp"], lv["Wt"], lv["gamma"], lv["beta"], 0.0,
                                 case.eps)
        y.backward(inp["dy"])
        keep, scale = _emb_mask(case)
        _, comp = cpu_embed(case, keep, scale)
        got = dict(comp, y=y.detach(), dWp=lv["Wp"].grad, dWt=lv["Wt"].grad, dgamma=lv["gamma"].grad,
                   dbeta=lv["beta"].grad, dWw=lv["Ww"].grad)
        check_embed(case, inp, got, keep, scale)
        break
    else:
        raise AssertionError("no fp32 p = 0 embedding case in the table")


def test_splitk_reference_and_fp32_sum():
    for n in R.SPLITK_N:
        for nsplit in R.SPLITK_NSPLIT:
            slabs, out0 = R.splitk_inputs(n, nsplit)
            for odt in (F32, F16, BF16):
                ref, cond, nt = R.ref_splitk(slabs)
                R.check_splitk(slabs.sum(0).to(odt), ref, cond, odt, nt, f"splitk n{n} s{nsplit}")
            ref, cond, nt = R.ref_splitk(slabs, out0)
            R.check_splitk(out0 + slabs.sum(0), ref, cond, F32, nt, "accumulate")
            with pytest.raises(AssertionError):   # mutant: accumulate ignored
                R.check_splitk(slabs.sum(0), ref, cond, F32, nt, "accumulate ignored")


# ----------------------------------------------------------------------------
# BOUNDS is what the CPU measures
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BDALN_CASES) + list(EMB_CASES))
def test_stats_bounds_are_the_measured_ones(name):
    s, eps = R.stats_input(name)
    for measured, bound, what in zip(R.measure_stats(s, eps), R.BOUNDS[name], ("mean", "rstd")):
        print(f"{name} {what}: measured {measured:.4e} recorded {bound:.3e}")
        assert measured <= bound <= 1.02 * measured, (name, what, measured, bound)


def test_bounds_table_has_no_stale_entries():
    assert set(R.BOUNDS) == set(BDALN_CASES) | set(EMB_CASES)


# ----------------------------------------------------------------------------
# float64 references against torch.autograd in float64
# ----------------------------------------------------------------------------
def _close(a, b, what):
    assert torch.allclose(a, b, rtol=1e-10, atol=1e-12), (what, float((a - b).abs().max()))


@pytest.mark.parametrize("act", R.ACTS)
def test_bias_act_reference_matches_autograd(act):
    g = torch.Generator().manual_seed(3 + act)
    x = (torch.randn((5, 8), generator=g, dtype=F64) * 2).requires_grad_(True)
    b = torch.randn((8,), generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn((5, 8), generator=g, dtype=F64)
    fops._act_ref(x + b, act).backward(dy)
    ref = R.ref_bias_act(x.detach(), b.detach(), dy, act)
    _close(ref["y"], fops._act_ref(x + b, act).detach(), "y")
    _close(ref["dx"], x.grad, "dx")
    _close(ref["db"], b.grad, "db")


@pytest.mark.parametrize("p,extra", [(0.0, False), (0.25, True), (0.25, False)])
def test_bdaln_reference_matches_autograd(p, extra):
    g = torch.Generator().manual_seed(17)
    rows, cols = 5, 16
    mk = lambda *s: torch.randn(s, generator=g, dtype=F64)
    x, res, dy, dse = mk(rows, cols), mk(rows, cols), mk(rows, cols), mk(rows, cols)
    bias, gamma, beta = mk(cols), 1 + 0.3 * mk(cols), mk(cols)
    th, scale = R.drop_params(p)
    keep = R.keep_mask(SEED, OFF, (rows, cols), th)
    lv = [t.clone().requires_grad_(True) for t in (x, bias, res, gamma, beta)]
    t = lv[0] + lv[1]
    s = lv[2] + torch.where(keep, t * scale, torch.zeros_like(t))
    y = F.layer_norm(s, (cols,), lv[3], lv[4], R.LN_EPS)
    loss = (y * dy).sum() + ((s * dse).sum() if extra else 0.0)
    loss.backward()
    inp = {"x": x, "bias": bias, "res": res, "dy": dy}
    s_ref, _ = R.ref_bdaln_s(inp, keep, scale)
    _close(s_ref, s.detach(), "s")
    fwd = R.ref_norm_fwd(s_ref, gamma, beta, R.LN_EPS, False)
    _close(fwd["y"], y.detach(), "y")
    bwd = R.ref_bdaln_bwd(dy, s_ref, gamma, beta, R.LN_EPS, keep, scale, dse if extra else None)
    for k, leaf in (("dx", lv[0]), ("dbias", lv[1]), ("dres", lv[2]), ("dgamma", lv[3]), ("dbeta", lv[4])):
        _close(bwd[k], leaf.grad, k)
    if not extra:   # the from-output formula is the same gradient
        fy = R.ref_bdaln_bwd_fromy(dy, y.detach(), gamma, beta, fwd["rstd"], keep, scale)
        for k in ("dx", "dres", "dgamma", "dbeta", "dbias"):
            assert torch.allclose(fy[k], bwd[k], rtol=1e-8, atol=1e-10), k


@pytest.mark.parametrize("types", R.EMB_TYPES)
def test_embedding_reference_matches_autograd(types):
    g = torch.Generator().manual_seed(23)
    B, S, H, V, npos, tv = 3, 4, 16, 9, 6, (1 if types == "tv1" else 2)
    mk = lambda *s: torch.randn(s, generator=g, dtype=F64)
    ids = torch.randint(0, V, (B, S), generator=g)
    tids = None if types == "none" else (torch.randint(0, tv, (B, S), generator=g))
    lv = [t.requires_grad_(True) for t in (mk(V, H), mk(npos, H), mk(tv, H), 1 + 0.3 * mk(H), mk(H))]
    dy = mk(B, S, H)
    th, scale = R.drop_params(0.25)
    keep = R.keep_mask(SEED, OFF, (B, S, H), th)
    y = fops.bert_embeddings(ids, tids, *lv, p=0.0, eps=R.LN_EPS)
    y = torch.where(keep, y * scale, torch.zeros_like(y))
    y.backward(dy)
    Ww, Wp, Wt, gamma, beta = [t.detach() for t in lv]
    s, _ = R.ref_embed_sum(ids, tids, Ww, Wp, Wt)
    fwd = R.ref_embed_fwd(s, gamma, beta, R.LN_EPS, keep, scale)
    _close(fwd["out"].reshape(B, S, H), y.detach(), "y")
    bwd = R.ref_embed_bwd(dy, fwd, s, tids, tv, npos, keep, scale, B, S)
    for k, leaf in (("dWp", lv[1]), ("dWt", lv[2]), ("dgamma", lv[3]), ("dbeta", lv[4])):
        _close(bwd[k], leaf.grad, k)
    dW, _, runs = R.ref_segsum(bwd["ds"].reshape(B * S, H), ids, V)
    _close(dW, lv[0].grad, "dWw")
    assert int(runs.sum()) == B * S


# ----------------------------------------------------------------------------
# the Python mask
# ----------------------------------------------------------------------------
def _mask_second(seed, offset, n, thresh, half_swap=False, per_element=False, offset32=False):
    """The same rule through attn_reference._philox4x32_7, one call per element, with the mutations."""
    e = np.arange(n, dtype=np.uint64)
    off = (offset & 0xFFFFFFFF) if offset32 else (offset & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        ctr = np.uint64(off) + (e if per_element else e // np.uint64(8))
        words = _philox4x32_7(seed, np.zeros_like(e), ctr)
    k = (e & np.uint64(7)).astype(np.int64)
    w = np.stack(words, 0)[k >> 1, np.arange(n)]
    high = (k & 1) == (0 if half_swap else 1)
    chunk = np.where(high, w >> np.uint64(16), w & np.uint64(0xFFFF))
    return torch.from_numpy(chunk >= np.uint64(thresh))


@pytest.mark.parametrize("cfg", ["base"] + list(R.CTR_CONFIGS))
@pytest.mark.parametrize("p", R.DROP_P + [0.25])
def test_mask_fraction_and_second_evaluation(cfg, p):
    seed, off = R.CTR_BASE if cfg == "base" else R.CTR_CONFIGS[cfg]
    th, scale = R.drop_params(p)
    n = 1 << 16
    keep = R.keep_mask(seed, off, (n,), th)
    q = 1.0 - th / 65536.0
    sigma = (n * q * (1 - q)) ** 0.5
    assert abs(int(keep.sum()) - n * q) <= 4 * sigma + 1e-9, (int(keep.sum()), n * q, sigma)
    assert torch.equal(keep, _mask_second(seed, off, n, th))
    assert scale == R.f32(1.0 / q)


def test_mask_edges():
    n = 1 << 16
    chunks = R.keep_chunks(*R.CTR_BASE, n)
    assert int(chunks.max()) < 65536
    keep1 = R.keep_mask(*R.CTR_BASE, (n,), 1)               # thresh 1: everything but the zero chunks
    assert torch.equal(keep1, torch.from_numpy(chunks != 0))
    th, scale = R.drop_params(1.0 - 2.0 ** -17)             # rounds to thresh 65536: nothing is kept
    assert th == 65536 and scale == INF
    keep = R.keep_mask(*R.CTR_BASE, (n,), th)
    assert not bool(keep.any())
    case = BDA_CASES["bda/f32-bf32-r17-c2056-p0.5"]
    x, b, res, dy = R.col_inputs(case)
    keep = R.keep_mask(*R.CTR_BASE, x.shape, th)
    ref = R.ref_bda(x, b, res, dy, keep, scale)
    for k in ("y", "dx", "db", "y_cond", "dx_cond", "db_cond"):
        assert bool(torch.isfinite(ref[k]).all()), k
    assert torch.equal(ref["y"], res.double()) and not bool(ref["dx"].any())
    y, dx, db = cpu_bda(case, keep, scale)
    assert torch.equal(y, res) and not bool(dx.any()) and not bool(db.any())
    assert R.drop_params(2.0 ** -18)[0] == 1 and R.drop_params(0.0) == (0, 1.0)


# ----------------------------------------------------------------------------
# mutants: each must be rejected on a table case
# ----------------------------------------------------------------------------
def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def test_mutant_erf_gelu_swapped_for_tanh():
    case = ACT_CASES["act/geluerf-f32-bf32-r17-c8"]
    _check_act(case, *cpu_bias_act(case))
    y, dx, db = cpu_bias_act(case, act=R.ACT_GELU_TANH)
    ref = R.act_reference(case.name)
    _rejects(lambda: R.check(y, ref["y"], ref["y_cond"], case.xdt))
    _rejects(lambda: R.check(dx, ref["dx"], ref["dx_cond"], case.xdt))


def test_mutant_unquantised_scale():
    """1 / (1 - p) for the quantised 1 / (1 - thresh / 65536): 6.8e-6 apart at p = 0.1. An elementwise output
    cannot tell them apart under C; the bias gradient of same-sign gradients does."""
    case = BDA_CASES["bda/f32-bf32-r33-c2056-p0.1-pos"]
    ref, keep = R.bda_reference(case, SEED, OFF)
    _check_bda(case, ref, *cpu_bda(case, keep, R.drop_params(case.p)[1]))
    y, dx, db = cpu_bda(case, keep, R.f32(1.0 / (1.0 - case.p)))
    _rejects(lambda: _check_bda(case, ref, y, dx, db))
    _rejects(lambda: R.check_colsum(db, ref["db"], ref["db_cond"], case.bdt, R.n_adds(case.rows)))


@pytest.mark.parametrize("mut,cfg", [("half_swap", "base"), ("per_element", "base"), ("offset32", "offhi")])
def test_mutant_masks(mut, cfg):
    """High and low halves swapped; counter e instead of e // 8; offset truncated to 32 bits."""
    case = BDA_CASES["bda/f16-bf16-r17-c2056-p0.5"]
    seed, off = R.CTR_BASE if cfg == "base" else R.CTR_CONFIGS[cfg]
    ref, keep = R.bda_reference(case, seed, off)
    th, scale = R.drop_params(case.p)
    _check_bda(case, ref, *cpu_bda(case, keep, scale))
    bad = _mask_second(seed, off, case.rows * case.cols, th, **{mut: True}).reshape(case.rows, case.cols)
    assert not torch.equal(bad, keep)
    y, dx, db = cpu_bda(case, bad, scale)
    _rejects(lambda: R.check(y, ref["y"], ref["y_cond"], case.xdt))
    _rejects(lambda: R.check(dx, ref["dx"], ref["dx_cond"], case.xdt))
    if mut == "offset32":   # on an offset below 2**32 the truncation is no mutant
        assert torch.equal(_mask_second(*R.CTR_BASE, 4096, th, offset32=True), R.keep_mask(*R.CTR_BASE, (4096,), th))


def _bdaln_mutant(name, mut, outs):
    case = BDALN_CASES[name]
    keep, scale = _ln_mask(case)
    inp, good = cpu_bdaln(case, keep, scale)
    check_bdaln(case, inp, good, keep, scale)
    _, bad = cpu_bdaln(case, keep, scale, mut)
    changed = [k for k in good if good[k] is not None and not torch.equal(good[k], bad[k])]
    assert set(outs) <= set(changed), (mut, changed)
    for k in outs:
        _rejects(lambda k=k: check_bdaln(case, inp, dict(good, **{k: bad[k]}), keep, scale))


def test_mutant_dbias_summed_before_the_mask():
    _bdaln_mutant("bdaln/f32-wf32-r5-c520-plain-p0.1", "dbias_before_mask", ["dbias"])


def test_mutant_mask_applied_to_dres():
    _bdaln_mutant("bdaln/f32-wf32-r5-c520-plain-p0.1", "mask_on_dres", ["dres"])


def test_mutant_ds_extra_left_out_of_dx():
    _bdaln_mutant("bdaln/f32-wf32-r5-c520-extra-p0.1", "extra_not_in_dx", ["dx", "dbias"])


def test_mutant_unbiased_variance():
    _bdaln_mutant("bdaln/f32-wf32-r5-c520-plain-p0", "unbiased_var", ["y", "dres"])


def test_mutant_layernorm_of_the_unrounded_s():
    _bdaln_mutant("bdaln/bf16-wbf16-r5-c520-plain-p0.1", "ln_unrounded_s", ["dres"])
    _bdaln_mutant("bdaln/f16-wf32-r5-c520-plain-p0.1", "ln_unrounded_s", ["dres"])


def test_mutant_second_rounding_of_y():
    _bdaln_mutant("bdaln/bf16-wbf16-r5-c520-plain-p0", "y_second_rounding", ["y"])
    _bdaln_mutant("bdaln/f16-wf32-r5-c520-plain-p0", "y_second_rounding", ["y"])


def test_mutant_from_output_dgamma_without_the_division():
    case = BDALN_CASES["bdaln/f32-wf32-r5-c520-plain-p0"]
    keep, scale = _ln_mask(case)
    inp, got = cpu_bdaln(case, keep, scale)
    ref = R.ref_bdaln_bwd_fromy(inp["dy"], got["y"], inp["gamma"], inp["beta"], got["rstd"], keep, scale)
    yc = got["y"].float() - inp["beta"].float()
    good = (inp["dy"].float() * yc).sum(0) / inp["gamma"].float()
    na = R.n_adds_ln(case.rows)
    R.check_colsum(good, ref["dgamma"], ref["dgamma_cond"], F32, na)
    _rejects(lambda: R.check_colsum((inp["dy"].float() * yc).sum(0), ref["dgamma"], ref["dgamma_cond"], F32, na))


def _emb_mutant(mut, out, pick):
    name = next(n for n, c in EMB_CASES.items() if pick(c))
    case = EMB_CASES[name]
    keep, scale = _emb_mask(case)
    inp, good = cpu_embed(case, keep, scale)
    check_embed(case, inp, good, keep, scale)
    _, bad = cpu_embed(case, keep, scale, mut)
    assert not torch.equal(bad[out], good[out])
    _rejects(lambda: check_embed(case, inp, dict(good, **{out: bad[out]}), keep, scale))


def test_mutant_type1_rows_summed_into_row0():
    _emb_mutant("type1_into_row0", "dWt", lambda c: c.types == "tv2" and c.B * c.S >= 4)


def test_mutant_segsum_drops_the_last_element_of_a_run():
    _emb_mutant("segsum_drops_last", "dWw", lambda c: c.ids == "equal" and c.B * c.S >= 3)
    _emb_mutant("segsum_drops_last", "dWw", lambda c: c.ids == "straddle" and c.B * c.S >= 12)
