"""CPU tier of the row-kernel checks: the package's fp32 CPU formulations (forward_torch_softmax,
softmax_xentropy on CPU tensors, F.layer_norm, _ref_rms) against the float64 reference of
tests/row_reference.py under its check(), on every case tests/test_row_kernels_gpu.py runs. That
shows the reference and the bound agree with an independent implementation, and it is where
row_reference.BOUNDS comes from. Then check() has to reject a set of subtly wrong results."""
import pytest
import torch
import torch.nn.functional as F

import row_reference as R

F32, F16, BF16 = R.F32, R.F16, R.BF16


def _pinned(measured, bound, what):
    """measured <= bound <= 1.02 * measured: the recorded bound is the measured figure rounded up
    in its third digit, nothing more (bound 0 exactly when nothing was measured)."""
    print(f"{what}: measured {measured:.4e} recorded {bound:.3e}")
    assert measured <= bound, (what, measured, bound)
    assert bound <= 1.02 * measured, (what, measured, bound)


# ----------------------------------------------------------------------------
# the fp32 CPU formulations
# ----------------------------------------------------------------------------
def mask_func(s, m):
    return s.masked_fill(m.bool(), -10000.0)


def cpu_softmax(case, x, mask):
    from apex.transformer.enums import AttnMaskType
    from apex.transformer.functional import FusedScaleMaskSoftmax

    mt = AttnMaskType.causal if case.mode == "causal" else AttnMaskType.padding
    m = FusedScaleMaskSoftmax(case.dtype == F16, case.dtype == BF16, mt, False, mask_func, True, case.scale)
    return m.forward_torch_softmax(x, mask)


def cpu_softmax_bwd(dy, y, scale):
    """dx = scale * y * (dy - sum(dy * y)) in fp32 from the stored y, rounded once."""
    dyf, yf = dy.float(), y.float()
    return (scale * yf * (dyf - (dyf * yf).sum(-1, keepdim=True))).to(y.dtype)


def cpu_xent(case, x, labels, dloss):
    """(lse, loss, dlogits): softmax_xentropy on CPU tensors in fp32, dlogits rounded once. The
    PyTorch path knows ignore_index only, so the out-of-range labels, which the kernel treats the
    same way, are renamed to it first."""
    from apex.contrib.xentropy.softmax_xentropy import softmax_xentropy

    lab = torch.where(R.xent_valid(labels, case.V, case.ignore_index), labels,
                      torch.full_like(labels, case.ignore_index))
    xf = x.float().clone().requires_grad_(True)
    rows = softmax_xentropy(xf, lab, case.smoothing, case.ignore_index, reduction="none")
    rows.backward(dloss)
    return torch.logsumexp(xf.detach(), -1), rows.detach(), xf.grad.to(case.dtype)


def cpu_norm(case, x, gamma, beta, dy):
    from apex.normalization.fused_layer_norm import _ref_rms

    xf = x.float().clone().requires_grad_(True)
    w = gamma.float().clone().requires_grad_(True) if gamma is not None else None
    b = beta.float().clone().requires_grad_(True) if beta is not None else None
    if case.rms:
        y = _ref_rms(xf, (case.cols,), w, case.eps)
    else:
        y = F.layer_norm(xf, (case.cols,), w, b, case.eps)
    y.backward(dy.float())
    return {"y": y.detach().to(case.xdt), "dx": xf.grad.to(case.xdt),
            "dgamma": w.grad.to(case.wdt) if w is not None else None,
            "dbeta": b.grad.to(case.wdt) if b is not None else None}


def cpu_norm_stats(case, x):
    """(mean, rstd) in fp32, the expressions of F.layer_norm and _ref_rms."""
    xf = x.float()
    if case.rms:
        return torch.zeros(case.rows), torch.rsqrt(xf.pow(2).mean(-1) + case.eps)
    return xf.mean(-1), torch.rsqrt(xf.var(-1, unbiased=False) + case.eps)


def measure_xent(case):
    x, labels, dloss = R.xent_inputs(case)
    lse, loss, _ = cpu_xent(case, x, labels, dloss)
    ref = R.ref_xent(x, labels, case.smoothing, case.ignore_index)
    return R.max_err(lse, ref["lse"]), R.max_err(loss, ref["loss"])


def measure_norm_stats(case):
    x = R.norm_inputs(case)[0]
    mean, rstd = cpu_norm_stats(case, x)
    ref = R.norm_reference(case.name)
    return R.max_err(mean, ref["mean"]), R.max_err(rstd, ref["rstd"])


# ----------------------------------------------------------------------------
# every case: fp32 CPU formulation inside the bound
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.SMX_CASES))
def test_cpu_softmax_inside_bound(name):
    case = R.SMX_CASES[name]
    x, dy, mask = R.smx_inputs(case)
    y = cpu_softmax(case, x, mask)
    assert y.dtype == case.dtype
    ref, cond = R.ref_softmax_fwd(x, case.scale, case.kernel_mode, mask)
    fw = R.check(y, ref, cond, case.dtype, name + " y")
    if case.mode == "causal":
        dead = torch.ones(case.sq, case.sk).triu(1).bool().expand(ref.shape)
        assert bool((ref[dead] == 0).all()) and bool((y[dead] == 0).all())
        assert bool((y[..., 0, 0] == 1).all())
    if case.mode == "maskh":
        assert bool((ref[-1, -1, -1] == 1.0 / case.sk).all())
    dx = cpu_softmax_bwd(dy, y, case.scale)
    rdx, cdx = R.ref_softmax_bwd(dy, y, case.scale)
    bw = R.check(dx, rdx, cdx, case.dtype, name + " dx")
    print(f"{name}: y {fw:.3f} dx {bw:.3f} of the bound")


@pytest.mark.parametrize("name", list(R.XENT_CASES))
def test_cpu_xentropy_inside_bound(name):
    case = R.XENT_CASES[name]
    x, labels, dloss = R.xent_inputs(case)
    lse, loss, dx = cpu_xent(case, x, labels, dloss)
    ref = R.ref_xent(x, labels, case.smoothing, case.ignore_index, dloss)
    assert bool(torch.isfinite(ref["loss"]).all()) and bool(torch.isfinite(ref["dlogits"]).all())
    dead = ~ref["valid"]
    assert int(dead.sum()) >= 3   # more where a drawn label happens to equal ignore_index
    assert bool((loss[dead] == 0).all()) and bool((dx[dead] == 0).all())
    assert bool((ref["loss"][dead] == 0).all()) and bool((ref["dlogits"][dead] == 0).all())
    e_lse, e_loss = R.max_err(lse, ref["lse"]), R.max_err(loss, ref["loss"])
    _pinned(e_lse, R.BOUNDS[name][0], name + " lse")
    _pinned(e_loss, R.BOUNDS[name][1], name + " loss")
    if case.kind in ("shift", "big"):
        return   # |x - lse| leaves the range C is derived for: the scalars alone are held to BOUNDS
    w = R.check(dx, ref["dlogits"], ref["dlogits_cond"], case.dtype, name + " dlogits")
    print(f"{name}: dlogits {w:.3f} of the bound")


@pytest.mark.parametrize("name", list(R.NORM_CASES))
def test_cpu_norm_inside_bound(name):
    case = R.NORM_CASES[name]
    x, gamma, beta, dy = R.norm_inputs(case)
    got = cpu_norm(case, x, gamma, beta, dy)
    ref = R.norm_reference(name)
    w = [R.check(got["y"], ref["y"], ref["y_cond"], case.xdt, name + " y"),
         R.check(got["dx"], ref["dx"], ref["dx_cond"], case.xdt, name + " dx")]
    if gamma is not None:
        w.append(R.check(got["dgamma"], ref["dgamma"], ref["dgamma_cond"], case.wdt, name + " dgamma"))
    if beta is not None:
        w.append(R.check(got["dbeta"], ref["dbeta"], ref["dbeta_cond"], case.wdt, name + " dbeta"))
    print(f"{name}: y, dx, dgamma, dbeta at", " ".join(f"{v:.3f}" for v in w), "of the bound")


@pytest.mark.parametrize("stats", sorted({c.stats for c in R.NORM_CASES.values()}))
def test_norm_stats_bounds_are_the_measured_ones(stats):
    case = next(c for c in R.NORM_CASES.values() if c.stats == stats)
    e_mean, e_rstd = measure_norm_stats(case)
    _pinned(e_mean, R.BOUNDS[stats][0], stats + " mean")
    _pinned(e_rstd, R.BOUNDS[stats][1], stats + " rstd")


def test_bounds_table_has_no_stale_entries():
    keys = set(R.XENT_CASES) | {c.stats for c in R.NORM_CASES.values()}
    assert set(R.BOUNDS) == keys


# ----------------------------------------------------------------------------
# -inf logits (a vocabulary padded to 50304 with the padding masked)
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_NAME.get)
def test_cpu_xentropy_with_masked_padding(dt):
    from apex.contrib.xentropy.softmax_xentropy import softmax_xentropy

    case = R.XENT_CASES[f"xent/{R.DT_NAME[dt]}-V50304-s0.0-ign-100-neginf"]
    x, labels, dloss = R.xent_inputs(case)
    assert bool((x[:, R.XENT_PAD_FROM:] == -R.INF).all()) and bool(torch.isfinite(x[:, :R.XENT_PAD_FROM]).all())
    lab = torch.where(R.xent_valid(labels, case.V, -100), labels, torch.full_like(labels, -100))
    rows = softmax_xentropy(x, lab, 0.0, -100, reduction="none")
    ref = R.ref_xent(x, labels, 0.0, -100, dloss)
    # the padding changes nothing: the same numbers as the 50257 real columns alone
    cut = R.ref_xent(x[:, :R.XENT_PAD_FROM], labels, 0.0, -100, dloss)
    assert R.max_err(ref["lse"], cut["lse"]) < 1e-13 and R.max_err(ref["loss"], cut["loss"]) < 1e-13
    assert bool((ref["dlogits"][:, R.XENT_PAD_FROM:] == 0).all())
    assert R.scalar_excess(rows, ref["loss"], R.BOUNDS[case.name][1]) <= 1.0


# ----------------------------------------------------------------------------
# check() rejects results that are subtly wrong
# ----------------------------------------------------------------------------
def _rejected(got, ref, cond, dtype):
    worst, _ = R.ratio(got, ref, cond, dtype)
    with pytest.raises(AssertionError, match="worst"):
        R.check(got, ref, cond, dtype, "mutant")
    return worst


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_NAME.get)
@pytest.mark.parametrize("sk", [64, 2048, 4096])
def test_check_rejects_zero_softmax(dt, sk):
    case = R.SMX_CASES[f"smx/{R.DT_NAME[dt]}-none-sk{sk}-sq{(1, 7)[R.SMX_SK.index(sk) % 2]}"]
    x, dy, _ = R.smx_inputs(case)
    ref, cond = R.ref_softmax_fwd(x, case.scale, "none")
    _rejected(torch.zeros_like(x), ref, cond, dt)
    y = cpu_softmax(case, x, None)
    rdx, cdx = R.ref_softmax_bwd(dy, y, case.scale)
    _rejected(torch.zeros_like(x), rdx, cdx, dt)


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_NAME.get)
@pytest.mark.parametrize("mode", ["mask1", "maskh", "causal"])
def test_check_rejects_softmax_that_ignores_its_mask(dt, mode):
    j = R.SMX_MODES.index(mode)
    sk = 1032
    case = R.SMX_CASES[f"smx/{R.DT_NAME[dt]}-{mode}-sk{sk}-sq{(1, 7)[(R.SMX_SK.index(sk) + j) % 2]}"]
    x, _, mask = R.smx_inputs(case)
    ref, cond = R.ref_softmax_fwd(x, case.scale, case.kernel_mode, mask)
    unmasked = R.ref_softmax_fwd(x, case.scale, "none")[0].to(dt)
    _rejected(unmasked, ref, cond, dt)


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_NAME.get)
def test_check_rejects_softmax_backward_without_dot(dt):
    case = R.SMX_CASES[f"smx/{R.DT_NAME[dt]}-none-sk512-sq7"]
    x, dy, _ = R.smx_inputs(case)
    y = cpu_softmax(case, x, None)
    rdx, cdx = R.ref_softmax_bwd(dy, y, case.scale)
    _rejected((case.scale * y.double() * dy.double()).to(dt), rdx, cdx, dt)


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_NAME.get)
@pytest.mark.parametrize("V", [8, 1000, 50257])
def test_check_rejects_dlogits_mutants(dt, V):
    case = next(c for c in R.XENT_CASES.values() if c.dtype == dt and c.V == V and c.smoothing > 0
                and c.kind == "plain" and not c.seed)
    x, labels, dloss = R.xent_inputs(case)
    ref = R.ref_xent(x, labels, case.smoothing, case.ignore_index, dloss)
    s = case.smoothing
    gv = torch.where(ref["valid"], dloss.double(), torch.zeros(R.XENT_N, dtype=torch.float64))[:, None]
    p = (x.double() - ref["lse"][:, None]).exp()
    safe = torch.where(ref["valid"], labels, torch.zeros_like(labels))
    hot = torch.zeros_like(p)
    hot[torch.arange(R.XENT_N), safe] = 1.0
    right = gv * (p - (1 - s) * hot - s / V)
    assert R.check(right.to(dt), ref["dlogits"], ref["dlogits_cond"], dt) <= 1.0
    # the label-smoothing term -s/V left out
    _rejected((gv * (p - (1 - s) * hot)).to(dt), ref["dlogits"], ref["dlogits_cond"], dt)
    # the one-hot one column off
    _rejected((gv * (p - (1 - s) * hot.roll(1, 1) - s / V)).to(dt), ref["dlogits"], ref["dlogits_cond"], dt)


@pytest.mark.parametrize("name", ["ln/bf16-wbf16-r5-c512", "ln/f32-wf32-r5-c64", "rms/f16-wf32-r5-c2560",
                                  "ln/bf16-wbf16-r3077-c64"])
def test_check_rejects_norm_mutants(name):
    case = R.NORM_CASES[name]
    x, gamma, beta, dy = R.norm_inputs(case)
    ref = R.norm_reference(name)
    # dgamma with one row left out
    dg = (dy.double() * ref["xhat"])[:-1].sum(0).to(case.wdt)
    _rejected(dg, ref["dgamma"], ref["dgamma_cond"], case.wdt)
    if not case.rms:
        db = dy.double()[1:].sum(0).to(case.wdt)
        _rejected(db, ref["dbeta"], ref["dbeta_cond"], case.wdt)
        # dx without the s1 = mean(dy g) term
        dyg = dy.double() * ref["g"]
        dx = ref["rstd"][:, None] * (dyg - ref["xhat"] * (dyg * ref["xhat"]).mean(-1, keepdim=True))
        _rejected(dx.to(case.xdt), ref["dx"], ref["dx_cond"], case.xdt)


def test_check_rejects_a_second_rounding():
    case = R.SMX_CASES["smx/f16-none-sk512-sq7"]
    x, _, _ = R.smx_inputs(case)
    ref, cond = R.ref_softmax_fwd(x, case.scale, "none")
    assert R.check(ref.float().half(), ref, cond, F16) <= 1.0
    _rejected(ref.float().bfloat16().half(), ref, cond, F16)
    ncase = R.NORM_CASES["ln/f16-wf16-r5-c520"]
    nref = R.norm_reference(ncase.name)
    assert R.check(nref["y"].float().half(), nref["y"], nref["y_cond"], F16) <= 1.0
    _rejected(nref["y"].float().bfloat16().half(), nref["y"], nref["y_cond"], F16)


def test_check_rejects_nonfinite_and_reports_the_index():
    ref = torch.ones(2, 3, dtype=torch.float64)
    got = ref.clone().float()
    got[1, 2] = float("nan")
    with pytest.raises(AssertionError, match=r"inf at \(1, 2\)"):
        R.check(got, ref, ref, F32, "nan")
