"""CPU tier: the float64 reference of tests/mt_reference.py against torch.optim in float64 and
against the project's fp32 CPU path (apex.multi_tensor_apply.ops, lamb_reference, LARC's CPU
branch), on the inputs tests/test_multi_tensor_gpu.py uses. The measured error of the fp32 path
is what the GPU tests' tolerances are built from (mt_reference.BOUNDS)."""
import math

import pytest
import torch

import mt_reference as R

F32, F16, BF16 = R.F32, R.F16, R.BF16


def _pinned(measured, bound, what):
    """measured <= bound <= 1.02 * measured: the recorded bound is the measured figure rounded up
    in its third digit, nothing more (bound 0 exactly when nothing was measured)."""
    print(f"{what}: measured {measured:.3e} recorded {bound:.3e}")
    assert measured <= bound, (what, measured, bound)
    assert bound <= 1.02 * measured, (what, measured, bound)


# ----------------------------------------------------------------------------
# the reference against independent float64 implementations
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("nesterov,dampening,wd", [(False, 0.0, 0.0), (True, 0.0, 0.1), (False, 0.1, 0.1)])
def test_reference_sgd_is_torch_sgd_in_float64(nesterov, dampening, wd):
    sizes = [1, 5, 1027]
    p = [t.double() for t in R.randn_list(sizes, 1)]
    q = [torch.nn.Parameter(t.clone()) for t in p]
    mom = [torch.zeros_like(t) for t in p]
    opt = torch.optim.SGD(q, lr=0.01, momentum=0.9, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    for k in range(3):
        g = [t.double() for t in R.randn_list(sizes, 10 + k)]
        R.ref_sgd_step(g, p, mom, lr=0.01, momentum=0.9, dampening=dampening, wd=wd, nesterov=nesterov,
                       first_run=(k == 0), wd_after_momentum=False)
        for x, gg in zip(q, g):
            x.grad = gg.clone()
        opt.step()
    for a, b in zip(p, q):
        torch.testing.assert_close(a, b.detach(), rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("adamw", [True, False])
def test_reference_adam_is_torch_adam_in_float64(adamw):
    sizes = [1, 5, 1027]
    p = [t.double() for t in R.randn_list(sizes, 2)]
    q = [torch.nn.Parameter(t.clone()) for t in p]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    opt = (torch.optim.AdamW if adamw else torch.optim.Adam)(q, lr=0.01, betas=(0.9, 0.999), eps=1e-8,
                                                             weight_decay=0.01)
    for k in range(3):
        g = [t.double() for t in R.randn_list(sizes, 20 + k)]
        R.ref_adam_step(g, p, m, v, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, step=k + 1, adamw=adamw,
                        bias_correction=True, wd=0.01)
        for x, gg in zip(q, g):
            x.grad = gg.clone()
        opt.step()
    # torch.optim folds the corrections differently (sqrt(v)/sqrt(bc2) + eps): equal in exact
    # arithmetic, a few float64 ulp apart
    for a, b in zip(p, q):
        torch.testing.assert_close(a, b.detach(), rtol=1e-12, atol=1e-13)


def test_reference_lamb_without_trust_ratio_or_clip_is_adam():
    sizes = [3, 1027]
    kw = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-6, bias_correction=True, wd=0.0, adamw=True)
    pa = [t.double() for t in R.randn_list(sizes, 3)]
    pl = [t.clone() for t in pa]
    ma, va, ml, vl = ([torch.zeros_like(t) for t in pa] for _ in range(4))
    for k in range(3):
        g = R.randn_list(sizes, 30 + k, BF16)
        R.ref_adam_step(g, pa, ma, va, step=k + 1, grad_scale=0.5, **kw)
        gn = R.ref_lamb_step(g, pl, ml, vl, step=k + 1, grad_scale=0.5, grad_averaging=True,
                             max_grad_norm=0.0, use_nvlamb=False, **kw)
        assert gn == pytest.approx(0.5 * math.sqrt(sum(float((t.double() ** 2).sum()) for t in g)), rel=1e-14)
    for a, b in zip(pa + ma + va, pl + ml + vl):
        assert torch.equal(a, b)


def test_reference_lamb_trust_ratio_and_clip_by_hand():
    """One tensor, one step, by hand: clip divides the gradient, the update has norm lr*||p||."""
    g = [torch.tensor([3.0, -4.0])]
    p = [torch.tensor([1.0, 2.0], dtype=torch.float64)]
    m, v = [torch.zeros(2, dtype=torch.float64)], [torch.zeros(2, dtype=torch.float64)]
    p0 = p[0].clone()
    gn = R.ref_lamb_step(g, p, m, v, lr=0.1, beta1=0.9, beta2=0.999, eps=0.0, step=1, bias_correction=True,
                         wd=0.0, grad_averaging=True, adamw=True, max_grad_norm=1.0, use_nvlamb=True)
    assert gn == 5.0
    torch.testing.assert_close(m[0], 0.1 * torch.tensor([0.6, -0.8], dtype=torch.float64), rtol=1e-14, atol=0)
    # u = sign(g) at step 1 with eps 0, ||u|| = sqrt(2); p -= lr * ||p||/||u|| * u
    want = p0 - 0.1 * math.sqrt(5.0) / math.sqrt(2.0) * torch.tensor([1.0, -1.0], dtype=torch.float64)
    torch.testing.assert_close(p[0], want, rtol=1e-14, atol=0)


def test_reference_larc_by_hand():
    g, p = [torch.tensor([3.0, 4.0]), torch.zeros(2)], [torch.tensor([0.0, 2.0]), torch.ones(2)]
    out = R.ref_larc_grads(g, p, trust=0.5, eps=0.0, lr=0.1, wd=0.5, clip=False)
    a = 0.5 * 2.0 / (5.0 + 2.0 * 0.5)
    torch.testing.assert_close(out[0], a * torch.tensor([3.0, 5.0], dtype=torch.float64), rtol=1e-15, atol=0)
    assert torch.equal(out[1], torch.zeros(2, dtype=torch.float64))
    out = R.ref_larc_grads(g, p, trust=0.5, eps=0.0, lr=0.1, wd=0.5, clip=True)
    torch.testing.assert_close(out[0], torch.tensor([3.0, 5.0], dtype=torch.float64), rtol=1e-15, atol=0)


# ----------------------------------------------------------------------------
# the project's fp32 CPU path against the reference: agreement, and the recorded bounds
# ----------------------------------------------------------------------------
def test_every_case_has_a_bound_and_sizes_cover_the_edges():
    assert set(R.BOUNDS) == set(R.CASES)
    assert R.SIZES_DEFAULT[0] == 0 and 32769 in R.SIZES_DEFAULT
    assert -(-R.SIZES_MANY[0] // R.SMALL_CHUNK) > 2048
    # one LAMB tensor spans 1, one 2 and one more than 2000 chunks
    assert {-(-n // R.DEFAULT_CHUNK) for n in R.SIZES_DEFAULT} >= {0, 1, 2, 3}


@pytest.mark.parametrize("case", R.LAMB_CASES, ids=lambda c: c.name)
def test_lamb_cases_clip_where_they_say_so(case):
    """max_grad_norm > 0 means an active clip in these cases: the norm the op works with (its own,
    or the supplied one) is above it at every step, whatever sizes and scale become later."""
    mgn = case.h["max_grad_norm"]
    assert mgn in (0.0, 1.0)
    _, grads = R.case_inputs(case)
    for gk in grads:
        norm = R.lamb_supplied_norm(case, gk) if case.h["supplied_norm"] else R.ref_l2norm(gk, case.scale)[0]
        assert norm > 2.0
    assert {c.h["max_grad_norm"] for c in R.LAMB_CASES} == {0.0, 1.0}


@pytest.mark.parametrize("key", sorted(R.CASES))
def test_cpu_path_agrees_with_reference_within_recorded_bound(key):
    case = R.CASES[key]
    got = R.run_case(case, "cpu")
    ref = R.reference(key)
    errs = R.state_errors(got, ref)
    for name, e, b in zip("pmv", errs, R.BOUNDS[key]):
        _pinned(e, b, f"{key} {name}")
    # fp32 rounding of O(1) state, nothing larger
    assert max(errs) < 1e-5, errs
    if case.cdt is not None:
        for c, p in zip(got["copy"], got["p"]):
            assert torch.equal(c, p.to(case.cdt))
    if case.op == "lamb":
        assert got["norm"] == pytest.approx(ref["norm"], rel=R.NORM_RTOL)


@pytest.mark.parametrize("clip,wd", R.LARC_CASES)
def test_larc_cpu_path_agrees_with_reference(clip, wd):
    from apex.parallel.LARC import LARC

    hp = R.LARC_HP
    gs, ps = R.larc_inputs(F32, F32)
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    for x, g in zip(params, gs):
        x.grad = g.clone()
    sgd = torch.optim.SGD(params, lr=hp["lr"], weight_decay=wd)
    LARC(sgd, trust_coefficient=hp["trust"], clip=clip, eps=hp["eps"]).step()
    assert sgd.param_groups[0]["weight_decay"] == wd
    ref_g = R.ref_larc_grads(gs, ps, wd=wd, clip=clip, **hp)
    ref_p = [p.double() - hp["lr"] * g for p, g in zip(ps, ref_g)]
    bg, bp = R.LARC_BOUNDS[(clip, wd != 0)]
    _pinned(R.max_abs_err([x.grad for x in params], ref_g), bg, f"larc clip={clip} wd={wd} grad")
    _pinned(R.max_abs_err(params, ref_p), bp, f"larc clip={clip} wd={wd} param")
    for i in (R.LARC_ZERO_GRAD, R.LARC_ZERO_PARAM):
        assert torch.equal(params[i].grad, gs[i])   # a zero norm leaves the gradient alone


@pytest.mark.parametrize("dt", R.DTYPES)
def test_cpu_scale_axpby_l2norm_agree_with_reference(dt):
    from apex.multi_tensor_apply import ops

    xs = R.randn_list(R.SIZES_DEFAULT, 5, dt)
    ys = R.randn_list(R.SIZES_DEFAULT, 6, F32)
    flag = torch.zeros(1, dtype=torch.int32)
    out = [torch.empty(x.numel()) for x in xs]
    ops.multi_tensor_scale(R.DEFAULT_CHUNK, flag, [xs, out], 0.125)
    for o, r in zip(out, R.ref_scale(xs, 0.125)):
        assert torch.equal(o.double(), r)   # one exact multiply
    ops.multi_tensor_axpby(R.DEFAULT_CHUNK, flag, [xs, ys, out], 0.5, -2.0, -1)
    ref = R.ref_axpby(xs, ys, 0.5, -2.0)
    extra = [2.0 ** -22 * (0.5 * x.double().abs() + 2.0 * y.double().abs()) for x, y in zip(xs, ys)]
    assert R.ulp_excess(out, ref, F32, extra) <= 1.0
    tot, per = ops.multi_tensor_l2norm(R.DEFAULT_CHUNK, flag, [xs], True)
    rt, rp = R.ref_l2norm(xs)
    assert float(tot) == pytest.approx(rt, rel=R.NORM_RTOL)
    assert per.tolist() == pytest.approx(rp, rel=R.NORM_RTOL)
    assert int(flag) == 0 and not R.ref_nonfinite(xs)
    xs[-1][-1] = float("nan")
    ops.multi_tensor_l2norm(R.DEFAULT_CHUNK, flag, [xs], False)
    assert int(flag) == 1 and R.ref_nonfinite(xs)


def test_fused_adam_cpu_legacy_clip_applies_with_amp_grad_scale():
    """FusedAdam's CPU branch: the legacy scale / clip factor and amp's gradient scale both apply
    (the device branch is checked in tests/test_multi_tensor_gpu.py)."""
    from apex.optimizers import FusedAdam

    case = R.CASES["adam/adamw-f32-clipamp"]
    h, c = case.h, R.ADAM_CLIP_AMP
    ps_c, grads_c = R.case_inputs(case)
    params = [torch.nn.Parameter(p) for p in ps_c]
    opt = FusedAdam(params, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], adam_w_mode=True,
                    weight_decay=h["wd"], max_grad_norm=c["max_grad_norm"])
    opt._amp_grad_scale = torch.tensor([c["amp_scale"]])
    for k in range(R.NSTEPS):
        opt.step(grads=grads_c[k], scale=c["scale"], grad_norms=c["norm"])
    ref = R.reference(case.key)
    got = {"p": [x.detach() for x in params], "m": [opt.state[x]["exp_avg"] for x in params],
           "v": [opt.state[x]["exp_avg_sq"] for x in params]}
    for e, b in zip(R.state_errors(got, ref), R.BOUNDS[case.key]):
        assert e <= R.MARGIN * b, (e, b)
