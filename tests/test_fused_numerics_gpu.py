"""The fused elementwise, residual-LayerNorm and embedding HIP kernels (csrc/fused_ops.hip) at the binding
level against the float64 references of fused_reference.py: every element of every output under the derived
bound, dropout masks equal to the Python mask, bit-exact integer cases, bit-identical reruns, caller-provided
outputs with guard bands, zero rows, and the refusals of the bindings (each an exception before any launch).

Shapes are the smallest that reach each path (fused_reference's case tables). The module prints the worst
|got - ref| / bound per kernel, output and dtype when it ends; with FUSED_NUMERICS_WORST_OUT set to a path it
also writes them there (profiles/fused_numerics_worst.txt is such a run)."""
import os

import pytest
import torch

import fused_reference as R
from fused_reference import (ACT_CASES, BDA_CASES, BDALN_CASES, BF16, EMB_CASES, F16, F32, INF, check_bdaln,
                             check_bdaln_bwd, check_embed)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -77.0


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    R.WORST.clear()
    yield
    lines = [f"  {tag}: {R.WORST[tag][0]:.3f}  ({R.WORST[tag][1]})" for tag in sorted(R.WORST)]
    print("\nworst |got - ref| / bound per kernel, output and dtype:")
    print("\n".join(lines))
    path = os.environ.get("FUSED_NUMERICS_WORST_OUT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def _C():
    from apex import _ext

    return _ext.require()


def _d(t):
    return t.to(DEV) if t is not None else None


def _configs(p):
    return [("base", R.CTR_BASE)] + (list(R.CTR_CONFIGS.items()) if p > 0 else [])


def _same(a, b):
    return (a is None and b is None) or (a.dtype == b.dtype and torch.equal(a, b))


# ----------------------------------------------------------------------------
# bias_act
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ACT_CASES))
def test_bias_act_case(name):
    C = _C()
    case = ACT_CASES[name]
    x_c, b_c, _, dy_c = R.col_inputs(case)
    x, b, dy = _d(x_c), _d(b_c), _d(dy_c)
    y = C.bias_act_fwd(x, b, case.act)
    dx, db = C.bias_act_bwd(dy, x, b, case.act)
    assert y.dtype == dx.dtype == case.xdt and y.shape == dx.shape == x.shape
    assert (db is None) == (b is None) and (db is None or (db.dtype == case.bdt and db.shape == b.shape))
    ref = R.act_reference(name)
    an = R.ACT_NAME[case.act]
    w = [R.check(y, ref["y"], ref["y_cond"], case.xdt, name + " y", f"bias_act {an}/y/{R.DT_NAME[case.xdt]}"),
         R.check(dx, ref["dx"], ref["dx_cond"], case.xdt, name + " dx", f"bias_act {an}/dx/{R.DT_NAME[case.xdt]}")]
    if b is not None:
        w.append(R.check_colsum(db, ref["db"], ref["db_cond"], case.bdt, R.n_adds(case.rows), name + " db",
                                f"bias_act {an}/db/{R.DT_NAME[case.bdt]}"))
    print(name + ":", " ".join(f"{v:.3f}" for v in w), "of the bound")
    if case.kind == "int":
        assert torch.equal(y.cpu().double(), ref["y"]) and torch.equal(dx.cpu().double(), ref["dx"])
        assert db is None or torch.equal(db.cpu().double(), ref["db"])
    assert torch.equal(x.cpu(), x_c) and torch.equal(dy.cpu(), dy_c), "an input was modified"
    dx2, db2 = C.bias_act_bwd(dy, x, b, case.act)
    assert torch.equal(C.bias_act_fwd(x, b, case.act), y) and torch.equal(dx2, dx) and _same(db2, db)


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("act", R.ACTS)
def test_bias_act_extreme_preactivations(dtype, act):
    """Pre-activations of +-30000: every output finite and inside the bound (every fp32 term of the formulas
    is finite there: x^3 = 2.7e13, exp(-x^2 / 2) = 0)."""
    C = _C()
    g = torch.Generator().manual_seed(5 + act)
    rows, cols = 17, 16
    sign = torch.where(torch.rand((rows, cols), generator=g) < 0.5, -1.0, 1.0)
    x_c = (30000.0 * sign).to(dtype)
    dy_c = (torch.rand((rows, cols), generator=g) + 0.5).to(dtype)
    b_c = torch.zeros(cols, dtype=dtype)
    y = C.bias_act_fwd(_d(x_c), _d(b_c), act)
    dx, db = C.bias_act_bwd(_d(dy_c), _d(x_c), _d(b_c), act)
    for t in (y, dx, db):
        assert bool(torch.isfinite(t.float()).all())
    ref = R.ref_bias_act(x_c, b_c, dy_c, act)
    for k in ("y", "dx", "db"):
        assert bool(torch.isfinite(ref[k]).all()) and bool(torch.isfinite(ref[k + "_cond"]).all())
    R.check(y, ref["y"], ref["y_cond"], dtype, "extreme y")
    R.check(dx, ref["dx"], ref["dx_cond"], dtype, "extreme dx")
    R.check_colsum(db, ref["db"], ref["db_cond"], dtype, R.n_adds(rows), "extreme db")


# ----------------------------------------------------------------------------
# bias_dropout_add, colsum
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BDA_CASES))
def test_bias_dropout_add_case(name):
    C = _C()
    case = BDA_CASES[name]
    x_c, b_c, res_c, dy_c = R.col_inputs(case)
    x, b, res, dy = _d(x_c), _d(b_c), _d(res_c), _d(dy_c)
    dn = R.DT_NAME[case.xdt]
    for cfg, (seed, off) in _configs(case.p):
        ref, keep = R.bda_reference(case, seed, off)
        y = C.bias_dropout_add_fwd(x, b, res, case.p, seed, off)
        dx, db = C.bias_dropout_add_bwd(dy, case.p, seed, off, b)
        assert y.dtype == dx.dtype == case.xdt and (db is None) == (b is None)
        what = f"{name} {cfg}"
        w = [R.check(y, ref["y"], ref["y_cond"], case.xdt, what + " y", f"bias_dropout_add/y/{dn}"),
             R.check(dx, ref["dx"], ref["dx_cond"], case.xdt, what + " dx", f"bias_dropout_add/dx/{dn}")]
        if b is not None:
            assert db.dtype == case.bdt and db.shape == b.shape
            w.append(R.check_colsum(db, ref["db"], ref["db_cond"], case.bdt, R.n_adds(case.rows), what + " db",
                                    f"bias_dropout_add/db/{R.DT_NAME[case.bdt]}"))
        print(what + ":", " ".join(f"{v:.3f}" for v in w), "of the bound")
        assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(dx.float()).all())
        # the zero pattern is the Python mask, forward (on a zero residual) and backward
        y0 = C.bias_dropout_add_fwd(x, b, torch.zeros_like(res), case.p, seed, off)
        assert torch.equal((y0 != 0).cpu(), keep), what + ": forward mask"
        assert torch.equal((dx != 0).cpu(), keep), what + ": backward mask"
        if case.kind == "int":
            assert torch.equal(y.cpu().double(), ref["y"]) and torch.equal(dx.cpu().double(), ref["dx"])
            assert db is None or torch.equal(db.cpu().double(), ref["db"])
        dx2, db2 = C.bias_dropout_add_bwd(dy, case.p, seed, off, b)
        assert torch.equal(C.bias_dropout_add_fwd(x, b, res, case.p, seed, off), y)
        assert torch.equal(dx2, dx) and _same(db2, db)
    assert torch.equal(x.cpu(), x_c) and torch.equal(res.cpu(), res_c) and torch.equal(dy.cpu(), dy_c)
    # colsum: the p = 0, no-dx launch of the same kernel
    odt = case.bdt if case.bdt is not None else F32
    cs = C.colsum(dy, odt)
    d64 = dy_c.double()
    assert cs.dtype == odt and cs.shape == (case.cols,)
    R.check_colsum(cs, d64.sum(0), d64.abs().sum(0), odt, R.n_adds(case.rows), name + " colsum",
                   f"colsum/{dn}/{R.DT_NAME[odt]}")
    if case.kind == "int":
        assert torch.equal(cs.cpu().double(), d64.sum(0))
    assert torch.equal(C.colsum(dy, odt), cs)


# ----------------------------------------------------------------------------
# splitk_reduce
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SPLITK_N)
@pytest.mark.parametrize("nsplit", R.SPLITK_NSPLIT)
def test_splitk_reduce(n, nsplit):
    C = _C()
    for integer in (False, True):
        slabs_c, out0_c = R.splitk_inputs(n, nsplit, integer)
        slabs = _d(slabs_c)
        for odt in (F32, F16, BF16):
            ref, cond, nt = R.ref_splitk(slabs_c)
            got = C.splitk_reduce(slabs, odt)
            assert got.dtype == odt and got.shape == (n,)
            R.check_splitk(got, ref, cond, odt, nt, f"splitk n{n} s{nsplit}", f"splitk_reduce/{R.DT_NAME[odt]}")
            if integer:
                assert torch.equal(got.cpu().double(), ref)
            assert torch.equal(C.splitk_reduce(slabs, odt), got)
        ref, cond, nt = R.ref_splitk(slabs_c, out0_c)
        out = _d(out0_c).clone()
        ret = C.splitk_reduce(slabs, F32, out, True)
        assert ret.data_ptr() == out.data_ptr()
        R.check_splitk(out, ref, cond, F32, nt, f"splitk accumulate n{n} s{nsplit}", "splitk_reduce accumulate/f32")
        if integer:
            assert torch.equal(out.cpu().double(), ref)
        assert torch.equal(slabs.cpu(), slabs_c)
    # a 2-d result and out= without accumulate: the pre-filled values are overwritten
    if n % 4 == 0 and n >= 8:
        slabs_c, _ = R.splitk_inputs(n, nsplit)
        out = torch.full((2, n // 2), SENTINEL, device=DEV)
        C.splitk_reduce(_d(slabs_c).view(nsplit, 2, n // 2), F32, out)
        ref, cond, nt = R.ref_splitk(slabs_c)
        R.check_splitk(out.view(-1), ref, cond, F32, nt, "splitk out=")


def test_splitk_reduce_refusals():
    C = _C()
    with pytest.raises(RuntimeError):   # n % 4 != 0 with more than one slab
        C.splitk_reduce(torch.zeros(2, 6, device=DEV), F32)
    C.splitk_reduce(torch.zeros(1, 6, device=DEV), F32)
    slabs = torch.zeros(2, 8, device=DEV)
    with pytest.raises(RuntimeError):   # accumulate with a 16-bit out
        C.splitk_reduce(slabs, BF16, torch.zeros(8, device=DEV, dtype=BF16), True)
    with pytest.raises(RuntimeError):   # accumulate without out
        C.splitk_reduce(slabs, F32, None, True)
    buf = torch.zeros(16, device=DEV)
    with pytest.raises(RuntimeError):   # out 4 bytes off a 16-byte boundary
        C.splitk_reduce(slabs, F32, buf[1:9])
    with pytest.raises(RuntimeError):   # slabs not fp32
        C.splitk_reduce(slabs.to(BF16), F32)
    assert not bool(buf.any())


# ----------------------------------------------------------------------------
# bdaln
# ----------------------------------------------------------------------------
def _bdaln_run(C, case, d, seed, off, **kw):
    y, s, mean, rstd = C.bdaln_fwd(d["x"], d["bias"], d["res"], d["gamma"], d["beta"], case.eps, case.p, seed, off)
    dres, dx, dg, dbeta, dbias = C.bdaln_bwd(d["dy"], s, d["gamma"], mean, rstd, case.p, seed, off,
                                             d["bias"] is not None, ds_extra=d["ds_extra"], **kw)
    return {"y": y, "s": s, "mean": mean, "rstd": rstd, "dres": dres, "dx": dx, "dgamma": dg, "dbeta": dbeta,
            "dbias": dbias}


def _assert_dx_mask(dx, dres, keep, what):
    """dx = keep scale ds next to dres = ds: nothing dropped is non-zero, and everything kept is non-zero unless
    ds itself rounded to zero (one element in millions does, in fp16)."""
    nz, dnz = (dx != 0).cpu(), (dres != 0).cpu()
    assert not bool((nz & ~keep).any()), what + ": a dropped element is not zero"
    assert not bool((keep & dnz & ~nz).any()), what + ": a kept element is zero"
    assert int((keep & ~nz).sum()) <= 2, what


def _assert_bdaln_types(case, got, has_bias):
    rc = (case.rows, case.cols)
    for k in ("y", "s", "dres", "dx"):
        assert got[k].dtype == case.xdt and tuple(got[k].shape) == rc, k
    for k in ("mean", "rstd"):
        assert got[k].dtype == F32 and tuple(got[k].shape) == (case.rows,), k
    for k in ("dgamma", "dbeta") + (("dbias",) if has_bias else ()):
        assert got[k].dtype == case.wdt and tuple(got[k].shape) == (case.cols,), k
    assert has_bias or got["dbias"] is None


@pytest.mark.parametrize("name", list(BDALN_CASES))
def test_bdaln_case(name):
    C = _C()
    case = BDALN_CASES[name]
    inp = R.bdaln_inputs(case)
    d = {k: _d(v) for k, v in inp.items()}
    th, scale = R.drop_params(case.p)
    has_bias = inp["bias"] is not None
    kind = "bdaln wide" if case.wide else "bdaln"
    for cfg, (seed, off) in _configs(case.p):
        keep = R.keep_mask(seed, off, (case.rows, case.cols), th)
        got = _bdaln_run(C, case, d, seed, off)
        _assert_bdaln_types(case, got, has_bias)
        if cfg != "base" and case.rows >= 1000:
            # the large-row cases pay for their float64 LayerNorm once: the other counter configurations check
            # what depends on the counter, s against its reference and the backward's zero pattern
            s_ref, s_cond = R.ref_bdaln_s(inp, keep, scale)
            R.check(got["s"], s_ref, s_cond, case.xdt, f"{name} {cfg} s", f"{kind}/s/{R.DT_NAME[case.xdt]}")
            _assert_dx_mask(got["dx"], got["dres"], keep, f"{name} {cfg}: backward mask")
            continue
        ratios = check_bdaln(case, inp, got, keep, scale, tagbase=kind, stats_bound=R.BOUNDS[name])
        print(f"{name} {cfg}:", " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
        for k in ("mean", "rstd"):
            tag = f"{kind}/{k} (scalar)"
            if ratios[k] > R.WORST.get(tag, (-1.0, ""))[0]:
                R.WORST[tag] = (ratios[k], name)
        _assert_dx_mask(got["dx"], got["dres"], keep, f"{name} {cfg}: backward mask")
        # store_s = False: the same y, mean and rstd, no s
        y2, s2, mean2, rstd2 = C.bdaln_fwd(d["x"], d["bias"], d["res"], d["gamma"], d["beta"], case.eps, case.p, seed,
                                           off, store_s=False)
        assert s2.numel() == 0 and torch.equal(y2, got["y"]) and torch.equal(mean2, got["mean"]) and \
            torch.equal(rstd2, got["rstd"])
        if case.wide or case.mode == "extra":
            with pytest.raises(RuntimeError):   # from-output: narrow rows, no ds_extra
                C.bdaln_bwd(d["dy"], y2, d["gamma"], mean2, rstd2, case.p, seed, off, has_bias,
                            ds_extra=d["ds_extra"], beta=d["beta"])
            continue
        fy = C.bdaln_bwd(d["dy"], y2, d["gamma"], mean2, rstd2, case.p, seed, off, has_bias, beta=d["beta"])
        fy = dict(zip(("dres", "dx", "dgamma", "dbeta", "dbias"), fy))
        ref = R.ref_bdaln_bwd_fromy(inp["dy"], y2.cpu(), inp["gamma"], inp["beta"], rstd2.cpu(), keep, scale, has_bias)
        check_bdaln_bwd(case, fy, ref, lambda o, dt: f"bdaln/{o}/{R.DT_NAME[dt]}", prefix="fromy ")
        _assert_dx_mask(fy["dx"], fy["dres"], keep, f"{name} {cfg}: from-output backward mask")
    for k, v in inp.items():
        assert v is None or torch.equal(d[k].cpu(), v), f"{k} was modified"
    again = _bdaln_run(C, case, d, seed, off)   # the last configuration once more: the same bits
    for k, v in got.items():
        assert _same(again[k], v), k


@pytest.mark.parametrize("cols", R.BDALN_BAD_COLS)
def test_bdaln_unsupported_cols_raise(cols):
    C = _C()
    rows = 3
    x = torch.zeros(rows, cols, device=DEV, dtype=BF16)
    v = torch.ones(cols, device=DEV, dtype=BF16)
    assert not C.bdaln_supported(cols) and not C.bdaln_wide_supported(cols)
    with pytest.raises(RuntimeError):
        C.bdaln_fwd(x, v, x, v, v, 1e-5, 0.0, 0, 0)
    st = torch.ones(rows, device=DEV)
    with pytest.raises(RuntimeError):
        C.bdaln_bwd(x, x, v, st, st, 0.0, 0, 0, True)


@pytest.mark.parametrize("zero", [False, True])
def test_bdaln_conditional_s(zero):
    """s_cond forward / s_alt backward: with a zero in gamma the forward stores s and the backward is the
    stored-input one; without, s stays unwritten and the backward is the from-output one."""
    C = _C()
    case = BDALN_CASES["bdaln/bf16-wbf16-r5-c520-plain-p0.1"]
    inp = R.bdaln_inputs(case)
    if zero:
        inp["gamma"][5] = 0
        inp["gamma"][case.cols - 3] = 0
    d = {k: _d(v) for k, v in inp.items()}
    seed, off = R.CTR_BASE
    th, scale = R.drop_params(case.p)
    keep = R.keep_mask(seed, off, (case.rows, case.cols), th)
    plain = _bdaln_run(C, case, d, seed, off)
    y, s2, mean, rstd = C.bdaln_fwd(d["x"], d["bias"], d["res"], d["gamma"], d["beta"], case.eps, case.p, seed, off,
                                    s_cond=True)
    assert torch.equal(y, plain["y"]) and torch.equal(mean, plain["mean"]) and torch.equal(rstd, plain["rstd"])
    assert s2.shape == plain["s"].shape and (not zero or torch.equal(s2, plain["s"]))
    alt = s2 if zero else torch.full_like(s2, 7.0)
    out = C.bdaln_bwd(d["dy"], y, d["gamma"], mean, rstd, case.p, seed, off, True, beta=d["beta"], s_alt=alt)
    got = dict(zip(("dres", "dx", "dgamma", "dbeta", "dbias"), out))
    for v in got.values():
        assert bool(torch.isfinite(v.float()).all())
    if zero:
        check_bdaln(case, inp, dict(plain, **got), keep, scale, tagbase="bdaln s_cond")
    else:
        ref = R.ref_bdaln_bwd_fromy(inp["dy"], y.cpu(), inp["gamma"], inp["beta"], rstd.cpu(), keep, scale)
        check_bdaln_bwd(case, got, ref, lambda o, dt: f"bdaln s_cond/{o}/{R.DT_NAME[dt]}", prefix="fromy ")


@pytest.mark.parametrize("name", ["bdaln/bf16-wbf16-r5-c520-plain-p0.1", "bdaln/f16-wf32-r5-c520-plain-p0",
                                  "bdaln/f32-wf32-r5-c520-plain-p0.1"])
@pytest.mark.parametrize("fmt", [0, 1])
def test_bdaln_fp8_side_output_variants(name, fmt):
    """q8_out on the forward, q8_out and q8_only on the backward: every non-code output under the plain
    kernel's bound (the codes themselves are test_fp8_gpu.py's)."""
    C = _C()
    case = BDALN_CASES[name]
    inp = R.bdaln_inputs(case)
    d = {k: _d(v) for k, v in inp.items()}
    seed, off = R.CTR_BASE
    th, scale = R.drop_params(case.p)
    keep = R.keep_mask(seed, off, (case.rows, case.cols), th)
    q = dict(q8_scale=torch.tensor([3.0], device=DEV), q8_fmt=fmt)
    codes = torch.zeros((case.rows, case.cols), device=DEV, dtype=torch.uint8)
    y, s, mean, rstd = C.bdaln_fwd(d["x"], d["bias"], d["res"], d["gamma"], d["beta"], case.eps, case.p, seed, off,
                                   q8_out=codes, q8_amax=torch.zeros(1, device=DEV), **q)
    fwd = {"y": y, "s": s, "mean": mean, "rstd": rstd}
    for from_y in (False, True):
        for only in (False, True):
            out = C.bdaln_bwd(d["dy"], y if from_y else s, d["gamma"], mean, rstd, case.p, seed, off, True,
                              beta=d["beta"] if from_y else None, q8_out=torch.zeros_like(codes),
                              q8_amax=torch.zeros(1, device=DEV), q8_only=only, **q)
            got = dict(zip(("dres", "dx", "dgamma", "dbeta", "dbias"), out))
            if only:
                got["dx"] = None   # allocated, not written
            tagbase = "bdaln q8" + (" only" if only else "")
            if from_y:
                ref = R.ref_bdaln_bwd_fromy(inp["dy"], y.cpu(), inp["gamma"], inp["beta"], rstd.cpu(), keep, scale)
                check_bdaln_bwd(case, got, ref, lambda o, dt: f"{tagbase}/{o}/{R.DT_NAME[dt]}", prefix="fromy ")
            else:
                check_bdaln(case, inp, dict(fwd, **got), keep, scale, tagbase=tagbase, stats_bound=R.BOUNDS[name])


@pytest.mark.parametrize("bdt", [BF16, F16])
def test_wrappers_with_16bit_bias_and_fp32_layernorm(bdt):
    """The usual mixed-precision layout through bias_dropout_add_ln and dense_bias_dropout_add_ln: the bias goes
    in as an exact fp32 copy and its gradient comes back in the bias's dtype, all against the float64 reference."""
    from apex.ops import fused as fops

    case = R.LnCase("wrapper", bdt, F32, 5, 520, "plain", 0.0)
    g = R._gen(f"wrapper-{R.DT_NAME[bdt]}")
    mk = lambda *s: torch.randn(s, generator=g)
    inp = {"x": mk(5, 520).to(bdt), "bias": mk(520).to(bdt), "res": mk(5, 520).to(bdt), "gamma": 1 + 0.5 * mk(520),
           "beta": mk(520), "dy": mk(5, 520).to(bdt), "ds_extra": None}
    keep = torch.ones((5, 520), dtype=torch.bool)
    outs = []
    for dense in (False, True):
        lv = {k: _d(inp[k]).clone().requires_grad_(True) for k in ("x", "bias", "res", "gamma", "beta")}
        if dense:
            y = fops.dense_bias_dropout_add_ln(lv["x"], torch.eye(520, device=DEV, dtype=bdt), lv["bias"], lv["res"],
                                               lv["gamma"], lv["beta"], 0.0, case.eps)
            s = None
        else:
            s, y = fops.bias_dropout_add_ln(lv["x"], lv["bias"], lv["res"], lv["gamma"], lv["beta"], 0.0, case.eps)
        y.backward(_d(inp["dy"]))
        assert lv["bias"].grad.dtype == bdt and lv["gamma"].grad.dtype == F32 and y.dtype == bdt
        outs.append({"s": s, "y": y.detach(), "dres": lv["res"].grad, "dx": lv["x"].grad, "dgamma": lv["gamma"].grad,
                     "dbeta": lv["beta"].grad, "dbias": lv["bias"].grad})
    got = dict(outs[0], s=outs[0]["s"].detach())
    dbias = got.pop("dbias")
    s_ref, s_cond = R.ref_bdaln_s(inp, keep, 1.0)
    R.check(got["s"], s_ref, s_cond, bdt, "wrapper s")
    s_st = got["s"].cpu()
    fwd = R.ref_norm_fwd(s_st, inp["gamma"], inp["beta"], case.eps, False)
    R.check(got["y"], fwd["y"], fwd["y_cond"], bdt, "wrapper y")
    bwd = R.ref_bdaln_bwd(inp["dy"], s_st, inp["gamma"], inp["beta"], case.eps, keep, 1.0)
    check_bdaln_bwd(case, dict(got, dbias=None), {k: v for k, v in bwd.items() if not k.startswith("dbias")})
    R.check_colsum(dbias, bwd["dbias"], bwd["dbias_cond"], bdt, R.n_adds_ln(5), "wrapper dbias")
    for k in ("y", "dres", "dx", "dgamma", "dbeta", "dbias"):   # x @ I is x: the same kernels on the same bits
        assert torch.equal(outs[1][k], outs[0][k]), k


# ----------------------------------------------------------------------------
# BERT embeddings
# ----------------------------------------------------------------------------
def _embed_run(C, case, d, seed, off, **outs):
    y, sv, mean, rstd = C.embed_ln_fwd(d["ids"], d["tids"], d["Ww"], d["Wp"], d["Wt"], d["gamma"], d["beta"],
                                       case.eps, case.p, seed, off)
    ds, dWp, dWt, dg, db = C.embed_ln_bwd(d["dy"], sv, d["gamma"], mean, rstd, d["tids"], case.tvocab, case.npos,
                                          case.p, seed, off, **{k: v for k, v in outs.items() if k != "out"})
    sorted_ids, perm = torch.sort(d["ids"].view(-1), stable=True)
    dWw = C.embed_segsum(ds, sorted_ids, perm, R.EMB_VOCAB, outs.get("out"))
    return {"y": y, "s": sv, "mean": mean, "rstd": rstd, "ds": ds, "dWp": dWp, "dWt": dWt, "dgamma": dg, "dbeta": db,
            "dWw": dWw}


@pytest.mark.parametrize("name", list(EMB_CASES))
def test_embedding_case(name):
    C = _C()
    case = EMB_CASES[name]
    inp = R.emb_inputs(case)
    d = {k: _d(v) for k, v in inp.items()}
    th, scale = R.drop_params(case.p)
    B, S, H = case.B, case.S, case.H
    for cfg, (seed, off) in _configs(case.p):
        keep = R.keep_mask(seed, off, (B, S, H), th)
        got = _embed_run(C, case, d, seed, off)
        assert got["y"].dtype == got["s"].dtype == got["ds"].dtype == got["dWw"].dtype == case.xdt
        assert got["dWp"].dtype == got["dWt"].dtype == case.xdt and got["dgamma"].dtype == got["dbeta"].dtype == case.wdt
        assert tuple(got["y"].shape) == (B, S, H) and tuple(got["dWp"].shape) == (case.npos, H)
        assert tuple(got["dWt"].shape) == (case.tvocab, H) and tuple(got["dWw"].shape) == (R.EMB_VOCAB, H)
        ratios = check_embed(case, inp, got, keep, scale, tagbase="embed", stats_bound=R.BOUNDS[name])
        print(f"{name} {cfg}:", " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
        for k in ("mean", "rstd"):
            tag = f"embed/{k} (scalar)"
            if ratios[k] > R.WORST.get(tag, (-1.0, ""))[0]:
                R.WORST[tag] = (ratios[k], name)
        assert torch.equal((got["y"] != 0).cpu(), keep), f"{name} {cfg}: forward mask"
        again = _embed_run(C, case, d, seed, off)
        for k, v in got.items():
            assert torch.equal(again[k], v), k
    for k, v in inp.items():
        assert v is None or torch.equal(d[k].cpu(), v), f"{k} was modified"


# ----------------------------------------------------------------------------
# caller-provided outputs, zero rows
# ----------------------------------------------------------------------------
class _Slots:
    """16-byte-aligned slices of one sentinel-filled buffer per dtype, with guard bands on both sides."""

    def __init__(self):
        self.bufs = []

    def take(self, n, dtype):
        pad = 64
        buf = torch.full((n + 2 * pad,), SENTINEL, device=DEV, dtype=dtype)
        out = buf[pad:pad + n]
        assert out.data_ptr() % 16 == 0
        self.bufs.append((buf, pad, n))
        return out

    def check(self):
        for buf, pad, n in self.bufs:
            assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all()), "guard band written"


def test_caller_provided_outputs():
    C = _C()
    slots = _Slots()
    # colsum, splitk_reduce
    case = BDA_CASES["bda/bf16-bf32-r17-c2056-p0.1"]
    _, _, _, dy_c = R.col_inputs(case)
    dy = _d(dy_c)
    o = slots.take(case.cols, F32)
    assert C.colsum(dy, F32, o).data_ptr() == o.data_ptr() and torch.equal(o, C.colsum(dy, F32))
    db_slot = slots.take(case.cols, F32)
    like = torch.zeros(case.cols, device=DEV)
    dx, db = C.bias_dropout_add_bwd(dy, case.p, 11, 3, like, db_slot)
    assert db.data_ptr() == db_slot.data_ptr() and torch.equal(db, C.bias_dropout_add_bwd(dy, case.p, 11, 3, like)[1])
    slabs = _d(R.splitk_inputs(2056, 7)[0])
    for odt in (F32, BF16):
        o = slots.take(2056, odt)
        C.splitk_reduce(slabs, odt, o)
        assert torch.equal(o, C.splitk_reduce(slabs, odt))
    # bdaln: dgamma / dbeta / dbias
    for name in ("bdaln/bf16-wbf16-r5-c520-plain-p0.1", "bdaln/f16-wf32-r5-c2056-plain-p0.1"):
        lc = BDALN_CASES[name]
        d = {k: _d(v) for k, v in R.bdaln_inputs(lc).items()}
        plain = _bdaln_run(C, lc, d, *R.CTR_BASE)
        o = {k: slots.take(lc.cols, lc.wdt) for k in ("dgamma_out", "dbeta_out", "dbias_out")}
        got = _bdaln_run(C, lc, d, *R.CTR_BASE, **o)
        for k in ("dgamma", "dbeta", "dbias"):
            assert got[k].data_ptr() == o[k + "_out"].data_ptr() and torch.equal(got[k], plain[k]), k
        assert torch.equal(got["dx"], plain["dx"]) and torch.equal(got["dres"], plain["dres"])
    # embedding: dWp / dWt / dgamma / dbeta and the word table
    name = next(n for n, c in EMB_CASES.items() if c.npos > c.S and c.tvocab == 2 and c.B >= 4)
    ec = EMB_CASES[name]
    d = {k: _d(v) for k, v in R.emb_inputs(ec).items()}
    plain = _embed_run(C, ec, d, *R.CTR_BASE)
    o = {"dwp_out": slots.take(ec.npos * ec.H, ec.xdt), "dwt_out": slots.take(ec.tvocab * ec.H, ec.xdt),
         "dgamma_out": slots.take(ec.H, ec.wdt), "dbeta_out": slots.take(ec.H, ec.wdt),
         "out": slots.take(R.EMB_VOCAB * ec.H, ec.xdt)}
    got = _embed_run(C, ec, d, *R.CTR_BASE, **o)
    for k, ok in (("dWp", "dwp_out"), ("dWt", "dwt_out"), ("dgamma", "dgamma_out"), ("dbeta", "dbeta_out"),
                  ("dWw", "out")):
        assert got[k].data_ptr() == o[ok].data_ptr() and torch.equal(got[k].reshape(-1), plain[k].reshape(-1)), k
    slots.check()


@pytest.mark.parametrize("with_out", [False, True])
def test_zero_rows_give_zero_reductions(with_out):
    """rows = 0 (B = 0 for the embedding): the launchers have nothing to run, so the bindings zero every reduced
    output, a caller's slot included (it would otherwise keep what the buffer held)."""
    C = _C()
    cols = 520
    slots = _Slots()
    take = (lambda n, dt: slots.take(n, dt)) if with_out else (lambda n, dt: None)
    e = torch.empty((0, cols), device=DEV, dtype=BF16)
    b = torch.ones(cols, device=DEV)
    outs = []
    dx, db = C.bias_act_bwd(e, e, b, 0)
    outs.append(db)
    o = take(cols, F32)
    outs.append(C.bias_dropout_add_bwd(e, 0.1, 11, 3, b, o)[1])
    assert o is None or outs[-1].data_ptr() == o.data_ptr()
    o = take(cols, F32)
    outs.append(C.colsum(e, F32, o))
    assert C.bias_act_fwd(e, b, 0).shape == (0, cols) and C.bias_dropout_add_fwd(e, b, e, 0.1, 11, 3).shape == (0, cols)
    st = torch.empty((0,), device=DEV)
    g16 = torch.ones(cols, device=DEV, dtype=BF16)
    y, s, mean, rstd = C.bdaln_fwd(e, g16, e, g16, g16, 1e-5, 0.1, 11, 3)
    assert y.shape == (0, cols) and mean.shape == (0,)
    for kw in ({}, {"beta": g16}):
        r = C.bdaln_bwd(e, e, g16, st, st, 0.1, 11, 3, True, dgamma_out=take(cols, BF16), dbeta_out=take(cols, BF16),
                        dbias_out=take(cols, BF16), **kw)
        assert r[0].shape == (0, cols)
        outs.extend(r[2:])
    S, H, npos = 5, 520, 8
    sv = torch.empty((0, S, H), device=DEV, dtype=BF16)
    r = C.embed_ln_bwd(sv, sv, g16, st, st, None, 2, npos, 0.1, 11, 3, dwp_out=take(npos * H, BF16),
                       dwt_out=take(2 * H, BF16), dgamma_out=take(H, BF16), dbeta_out=take(H, BF16))
    assert r[0].shape == (0, S, H)
    outs.extend(r[1:])
    ids = torch.empty((0, S), device=DEV, dtype=torch.int32)
    tab = torch.ones((npos, H), device=DEV, dtype=BF16)
    assert C.embed_ln_fwd(ids, None, tab, tab, tab[:2], g16, g16, 1e-5, 0.0, 0, 0)[0].shape == (0, S, H)
    outs.append(C.embed_segsum(sv, ids.view(-1), torch.empty((0,), device=DEV, dtype=torch.int64), 9, take(9 * H, BF16)))
    torch.cuda.synchronize()
    for i, t in enumerate(outs):
        assert t.numel() > 0 and not bool(t.any()), f"output {i} is not zero"
    slots.check()


# ----------------------------------------------------------------------------
# operand refusals: every one raises before any launch
# ----------------------------------------------------------------------------
def _in_big(shape, dtype, device=DEV):
    """A tensor of `shape` that is a view into a buffer four times the bytes an fp32 tensor of that shape takes."""
    n = 1
    for v in shape:
        n *= v
    return torch.zeros(16 * max(n, 1), dtype=torch.uint8, device=device).view(dtype)[:n].view(shape)


def _wrongs(shape, dtype):
    """Mismatched stand-ins for a `dtype` tensor of `shape`: another dtype, another size, another device, and
    non-contiguous, each inside a generous allocation."""
    other = F32 if dtype != F32 else BF16
    bigger = tuple(shape[:-1]) + (shape[-1] + 8,)
    nc = _in_big(tuple(shape[:-1]) + (2 * shape[-1],), dtype)[..., ::2]
    assert not nc.is_contiguous() or nc.numel() <= 1
    return {"dtype": _in_big(shape, other), "size": _in_big(bigger, dtype), "device": _in_big(shape, dtype, "cpu"),
            "noncontiguous": nc}


def _refuses(fn, args, pos, shape, dtype, kinds=("dtype", "size", "device", "noncontiguous"), kwargs=None):
    w = _wrongs(shape, dtype)
    for kind in kinds:
        a = list(args)
        kw = dict(kwargs or {})
        if isinstance(pos, int):
            a[pos] = w[kind]
        else:
            kw[pos] = w[kind]
        with pytest.raises(RuntimeError):
            fn(*a, **kw)


def test_operand_refusals():
    C = _C()
    rows, cols = 5, 520
    x = torch.zeros((rows, cols), device=DEV, dtype=BF16)
    v16 = torch.ones(cols, device=DEV, dtype=BF16)
    v32 = torch.ones(cols, device=DEV)
    st = torch.ones(rows, device=DEV)
    rc, c = (rows, cols), (cols,)
    # bias_act: x non-contiguous (forward and backward), dy, bias size / device
    _refuses(C.bias_act_fwd, (x, v16, 0), 0, rc, BF16, ("device", "noncontiguous"))
    _refuses(C.bias_act_fwd, (x, v16, 0), 1, c, BF16, ("size", "device", "noncontiguous"))
    _refuses(C.bias_act_bwd, (x, x, v16, 0), 1, rc, BF16, ("device", "noncontiguous"))
    _refuses(C.bias_act_bwd, (x, x, v16, 0), 0, rc, BF16, ("dtype", "size", "device"))
    _refuses(C.bias_act_bwd, (x, x, v16, 0), 2, c, BF16, ("size", "device", "noncontiguous"))
    # bias_dropout_add
    _refuses(C.bias_dropout_add_fwd, (x, v16, x, 0.0, 0, 0), 2, rc, BF16)
    _refuses(C.bias_dropout_add_fwd, (x, v16, x, 0.0, 0, 0), 1, c, BF16, ("size", "device", "noncontiguous"))
    _refuses(C.bias_dropout_add_bwd, (x, 0.0, 0, 0, v16), 4, c, BF16, ("size", "device"))
    _refuses(C.bias_dropout_add_bwd, (x, 0.0, 0, 0, v16), 0, rc, BF16, ("device",))
    _refuses(C.colsum, (x, F32), 0, rc, BF16, ("device",))
    # bdaln forward: the bias must have gamma's dtype (the kernel reads it through gamma's type)
    fwd = (x, v32, x, v32, v32, 1e-5, 0.0, 0, 0)
    C.bdaln_fwd(*fwd)
    _refuses(C.bdaln_fwd, fwd, 1, c, F32)
    _refuses(C.bdaln_fwd, fwd, 2, rc, BF16)
    _refuses(C.bdaln_fwd, fwd, 3, c, F32, ("size", "device", "noncontiguous"))
    _refuses(C.bdaln_fwd, fwd, 4, c, F32)
    _refuses(C.bdaln_fwd, fwd, 0, rc, BF16, ("device", "noncontiguous"))
    with pytest.raises(RuntimeError):   # 16-bit bias next to fp32 gamma, in an allocation large enough for fp32
        C.bdaln_fwd(x, _in_big(c, BF16), x, v32, v32, 1e-5, 0.0, 0, 0)
    with pytest.raises(RuntimeError):   # fp32 bias next to 16-bit gamma
        C.bdaln_fwd(x, v32, x, v16, v16, 1e-5, 0.0, 0, 0)
    # bdaln backward
    bwd = (x, x, v32, st, st, 0.0, 0, 0, True)
    r = C.bdaln_bwd(*bwd)
    assert r[4].dtype == F32   # the bias gradient in the bias's (= gamma's) dtype
    _refuses(C.bdaln_bwd, bwd, 0, rc, BF16, ("dtype", "size", "device"))
    _refuses(C.bdaln_bwd, bwd, 1, rc, BF16, ("device", "noncontiguous"))
    _refuses(C.bdaln_bwd, bwd, 2, c, F32, ("size", "device", "noncontiguous"))
    _refuses(C.bdaln_bwd, bwd, 3, (rows,), F32)
    _refuses(C.bdaln_bwd, bwd, 4, (rows,), F32)
    _refuses(C.bdaln_bwd, bwd, "ds_extra", rc, BF16, ("dtype", "size", "device"))
    _refuses(C.bdaln_bwd, bwd, "beta", c, F32)
    _refuses(C.bdaln_bwd, bwd, "s_alt", rc, BF16, ("dtype", "device", "noncontiguous"), kwargs={"beta": v32})
    _refuses(C.bdaln_bwd, bwd, "dbias_out", c, F32)
    # embedding
    B, S, H, V = 3, 5, 520, 9
    ids = torch.zeros((B, S), device=DEV, dtype=torch.int32)
    tab = torch.ones((V, H), device=DEV, dtype=BF16)
    g = torch.ones(H, device=DEV)
    ef = (ids, ids, tab, tab, tab[:2], g, g, 1e-5, 0.0, 0, 0)
    y, sv, mean, rstd = C.embed_ln_fwd(*ef)
    _refuses(C.embed_ln_fwd, ef, 5, (H,), F32, ("size", "device", "noncontiguous"))
    _refuses(C.embed_ln_fwd, ef, 6, (H,), F32)
    _refuses(C.embed_ln_fwd, ef, 2, (V, H), BF16, ("dtype", "device", "noncontiguous"))
    _refuses(C.embed_ln_fwd, ef, 3, (V, H), BF16, ("dtype", "device", "noncontiguous"))
    _refuses(C.embed_ln_fwd, ef, 4, (2, H), BF16, ("dtype", "device", "noncontiguous"))
    _refuses(C.embed_ln_fwd, ef, 1, (B, S), torch.int32, ("size", "device", "noncontiguous"))
    eb = (y, sv, g, mean, rstd, ids, 2, S, 0.0, 0, 0)
    C.embed_ln_bwd(*eb)
    _refuses(C.embed_ln_bwd, eb, 0, (B, S, H), BF16, ("dtype", "size", "device"))
    _refuses(C.embed_ln_bwd, eb, 1, (B, S, H), BF16, ("device", "noncontiguous"))
    _refuses(C.embed_ln_bwd, eb, 2, (H,), F32, ("size", "device", "noncontiguous"))
    _refuses(C.embed_ln_bwd, eb, 3, (B * S,), F32)
    _refuses(C.embed_ln_bwd, eb, 4, (B * S,), F32)
    _refuses(C.embed_ln_bwd, eb, 5, (B, S), torch.int32, ("size", "device", "noncontiguous"))
    with pytest.raises(RuntimeError):   # type ids as int64
        C.embed_ln_bwd(y, sv, g, mean, rstd, _in_big((B, S), torch.int64), 2, S, 0.0, 0, 0)
    for bad in (dict(tvocab=3), dict(tvocab=0), dict(npos=S - 1)):
        with pytest.raises(RuntimeError):
            C.embed_ln_bwd(y, sv, g, mean, rstd, ids, bad.get("tvocab", 2), bad.get("npos", S), 0.0, 0, 0)
    sid, perm = torch.sort(ids.view(-1), stable=True)
    sg = (sv, sid, perm, V)
    C.embed_segsum(*sg)
    _refuses(C.embed_segsum, sg, 0, (B, S, H), BF16, ("device", "noncontiguous"))
    _refuses(C.embed_segsum, sg, 1, (B * S,), torch.int32, ("size", "device", "noncontiguous"))
    _refuses(C.embed_segsum, sg, 2, (B * S,), torch.int64, ("size", "device", "noncontiguous"))
    torch.cuda.synchronize()
