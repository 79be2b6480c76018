"""Every code path of csrc/multi_tensor.hip against the float64 reference of tests/mt_reference.py.

Paths, and how a test knows it took one: the vector path and the scalar path (plan.aligned 1 / 0,
tensors placed one element off a 16-byte boundary), one chunk, several chunks and more than
kMaxGrid = 2048 chunks (chunk_size 64, plan.nchunks asserted, so the grid-stride loop wraps), the
three sweeps of stream_for and the two of chunk_for (size sets in mt_reference), every dtype
instantiation the optimizers use, device and host gradient scales, device step counters and the
skip flag.

Tolerances: fp32 state is held to MARGIN (4) times the measured error of the project's fp32 CPU
path against the same reference on the same inputs (mt_reference.BOUNDS, measured and pinned by
tests/test_mt_reference.py); norms to rtol 1e-4; 16-bit outputs to one rounding of the float64
result; copies and skipped steps exactly. Every test prints its figures before asserting.
"""
import pytest
import torch

import mt_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F16, BF16 = R.F32, R.F16, R.BF16
INF, NAN = float("inf"), float("nan")


def _ids(v):
    return R.DT_NAME.get(v) if isinstance(v, torch.dtype) or v is None else None


def _ops():
    from apex.multi_tensor_apply import get_plan, ops

    return get_plan, ops


def _flag(v=0):
    return torch.full((1,), v, dtype=torch.int32, device=DEV)


def _check_plan(lists, chunk, sizes, place):
    """The path this test took: alignment flag and chunk count of the plan the op used."""
    get_plan, _ = _ops()
    plan = get_plan(lists, chunk)
    assert plan.aligned == (1 if place == "aligned" else 0), (place, plan.aligned)
    if sizes == "many":
        assert plan.nchunks > 2048, plan.nchunks
    return plan


# size set x placement: vector path, scalar path, grid-stride loop
LAYOUTS = [("default", "aligned"), ("default", "unaligned"), ("default", "mixed"), ("many", "aligned")]
LAYOUT_IDS = ["-".join(x) for x in LAYOUTS]


# ----------------------------------------------------------------------------
# scale
# ----------------------------------------------------------------------------
def _run_scale(xs_c, dout, place, chunk, scale, tensor_scale=False, inplace=False):
    _, ops = _ops()
    xs = R.put(xs_c, DEV, place)
    ys = xs if inplace else R.put([torch.zeros(x.numel(), dtype=dout) for x in xs_c], DEV, place)
    flag = _flag()
    ops.multi_tensor_scale(chunk, flag, [xs, ys],
                           torch.tensor([scale], device=DEV) if tensor_scale else scale)
    assert int(flag) == 0
    return xs, ys


def _assert_scaled(ys, xs_c, s, dout):
    ref = R.ref_scale(xs_c, s)
    if dout == F32:
        # the double product of two fp32 numbers is exact, so its rounding to fp32 IS the fp32 product
        for y, r in zip(ys, ref):
            assert torch.equal(y.cpu(), r.float())
    else:
        ex = R.ulp_excess(ys, ref, dout, [R.HALF_ULP[F32] * r.abs() for r in ref])
        print("scale: error / (one rounding to", dout, ") =", ex)
        assert ex <= 1.0


@pytest.mark.parametrize("sizes,place", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dout", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("din", R.DTYPES, ids=_ids)
def test_scale_matches_reference(din, dout, sizes, place):
    sizelist, chunk = R.SIZE_SETS[sizes]
    s = R.f32(0.3)
    xs_c = R.randn_list(sizelist, 11, din)
    xs, ys = _run_scale(xs_c, dout, place, chunk, s)
    _check_plan([xs, ys], chunk, sizes, place)
    _assert_scaled(ys, xs_c, s, dout)
    for x, c in zip(xs, xs_c):
        assert torch.equal(x.cpu(), c)   # the input list is only read
    if din == dout:   # in place, as amp's unscale_and_update does
        g, g2 = _run_scale(xs_c, dout, place, chunk, s, inplace=True)
        assert g is g2
        for a, b in zip(g, ys):
            assert torch.equal(a, b)


@pytest.mark.parametrize("dout", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("din", R.DTYPES, ids=_ids)
def test_scale_is_bit_identical_on_every_path(din, dout):
    """One multiply per element: vector and scalar path, chunk 32768 and 64, float and device
    scale must give the same bits."""
    s = R.f32(0.3)
    xs_c = R.randn_list(R.SIZES_DEFAULT, 12, din)
    _, base = _run_scale(xs_c, dout, "aligned", R.DEFAULT_CHUNK, s)
    _assert_scaled(base, xs_c, s, dout)   # the baseline itself against the float64 reference
    for place, chunk, tensor_scale in [("unaligned", R.DEFAULT_CHUNK, False), ("aligned", R.SMALL_CHUNK, False),
                                       ("aligned", R.DEFAULT_CHUNK, True), ("unaligned", R.SMALL_CHUNK, True)]:
        _, ys = _run_scale(xs_c, dout, place, chunk, s, tensor_scale)
        for a, b in zip(base, ys):
            assert torch.equal(a, b), (place, chunk, tensor_scale)


# ----------------------------------------------------------------------------
# overflow flag: scale, axpby, l2norm
# ----------------------------------------------------------------------------
OVF_SIZES = [5123, 36867, 4099]
# (tensor, element, which part of the sweep reads it)
OVF_POS = [(0, 0, "element 0"),
           (0, 2000, "4096-element unrolled body"),
           (0, 4500, "1024-element stride remainder"),
           (0, 5122, "scalar tail (n % 4 == 3)"),
           (1, 32768 + 4098, "last element of the last chunk of a two-chunk tensor"),
           (2, 17, "last tensor")]


def _ovf_runner(op, dt, place, check=-1):
    _, ops = _ops()
    xs = R.put(R.randn_list(OVF_SIZES, 21, dt), DEV, place)
    ys = R.put(R.randn_list(OVF_SIZES, 22, dt), DEV, place)
    out = R.put([torch.zeros(n, dtype=dt) for n in OVF_SIZES], DEV, place)
    flag = _flag()

    def run(check=check):
        flag.zero_()
        if op == "scale":
            ops.multi_tensor_scale(R.DEFAULT_CHUNK, flag, [xs, out], 0.5)
        elif op == "axpby":
            ops.multi_tensor_axpby(R.DEFAULT_CHUNK, flag, [xs, ys, out], 0.5, 2.0, check)
        else:
            ops.multi_tensor_l2norm(R.DEFAULT_CHUNK, flag, [xs], True)
        return int(flag)

    return xs, ys, run


@pytest.mark.parametrize("place", ["aligned", "unaligned"])
@pytest.mark.parametrize("bad", [INF, NAN], ids=["inf", "nan"])
@pytest.mark.parametrize("dt", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("op", ["scale", "axpby", "l2norm"])
def test_overflow_flag_at_every_position(op, dt, bad, place):
    xs, _, run = _ovf_runner(op, dt, place)
    assert run() == 0, "all-finite input raised the flag"
    for t, i, where in OVF_POS:
        keep = xs[t][i].clone()
        xs[t][i] = bad
        assert run() == 1, f"{bad} in the {where} not flagged"
        xs[t][i] = keep
    assert run() == 0


@pytest.mark.parametrize("dt", R.DTYPES, ids=_ids)
def test_axpby_checks_only_the_requested_argument(dt):
    xs, ys, run = _ovf_runner("axpby", dt, "aligned")
    ys[1][36000] = INF
    assert run(0) == 0 and run(1) == 1 and run(-1) == 1
    ys[1][36000] = 0.0
    xs[2][4098] = INF
    assert run(1) == 0 and run(0) == 1 and run(-1) == 1


# ----------------------------------------------------------------------------
# axpby
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,place", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dx,dy,do", [(BF16, F32, F32), (F16, F16, F16), (F32, F32, BF16)],
                         ids=["bf16.f32-f32", "f16.f16-f16", "f32.f32-bf16"])
def test_axpby_matches_reference(dx, dy, do, sizes, place):
    _, ops = _ops()
    sizelist, chunk = R.SIZE_SETS[sizes]
    sizelist = sizelist + (R.SIZES_AXPBY_EDGES if sizes == "default" else [])
    a, b = R.f32(0.3), R.f32(-1.7)
    xs_c, ys_c = R.randn_list(sizelist, 31, dx), R.randn_list(sizelist, 32, dy)
    xs, ys = R.put(xs_c, DEV, place), R.put(ys_c, DEV, place)
    out = R.put([torch.zeros(n, dtype=do) for n in sizelist], DEV, place)
    flag = _flag()
    ops.multi_tensor_axpby(chunk, flag, [xs, ys, out], a, b, -1)
    _check_plan([xs, ys, out], chunk, sizes, place)
    assert int(flag) == 0
    ref = R.ref_axpby(xs_c, ys_c, a, b)
    # fp32 evaluation of a*x + b*y: two products and a sum, each within 2^-24 relative
    extra = [2.0 ** -22 * ((a * x.double()).abs() + (b * y.double()).abs()) for x, y in zip(xs_c, ys_c)]
    ex = R.ulp_excess(out, ref, do, extra)
    print("axpby: error / (fp32 evaluation + one rounding to", do, ") =", ex)
    assert ex <= 1.0


# ----------------------------------------------------------------------------
# l2norm
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,place", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("mode", ["ops", "float-scale", "tensor-scale"])
@pytest.mark.parametrize("dt", R.DTYPES, ids=_ids)
def test_l2norm_matches_reference(dt, mode, sizes, place):
    get_plan, ops = _ops()
    sizelist, chunk = R.SIZE_SETS[sizes]
    xs_c = R.randn_list(sizelist, 41, dt)
    xs = R.put(xs_c, DEV, place)
    flag = _flag()
    s = 1.0 if mode == "ops" else R.f32(1.0 / 96)
    if mode == "ops":
        tot, per = ops.multi_tensor_l2norm(chunk, flag, [xs], True)
        tot2, per2 = ops.multi_tensor_l2norm(chunk, flag, [xs], False)
        assert per2.numel() == 0 and torch.equal(tot, tot2)
    elif mode == "float-scale":
        tot, per = get_plan([xs], chunk).l2norm(0, True, None, s, flag)
    else:
        tot, per = get_plan([xs], chunk).l2norm(0, True, torch.tensor([s], device=DEV), 1.0, flag)
    _check_plan([xs], chunk, sizes, place)
    assert int(flag) == 0
    rt, rp = R.ref_l2norm(xs_c, s)
    print("l2norm global", float(tot), "ref", rt)
    assert float(tot) == pytest.approx(rt, rel=R.NORM_RTOL)
    assert per.tolist() == pytest.approx(rp, rel=R.NORM_RTOL)
    for n, v in zip(sizelist, per.tolist()):
        if n == 0:
            assert v == 0.0   # an empty tensor has norm 0


# ----------------------------------------------------------------------------
# SGD / Adam / LAMB through the ops entry points (LAMB: the plan's lamb)
# ----------------------------------------------------------------------------
def _assert_state(case, got, ref, what=""):
    errs = R.state_errors(got, ref)
    bounds = R.BOUNDS[case.key]
    print(f"{case.key} {what}: |err| p, m, v = " + ", ".join(f"{e:.3e}" for e in errs) +
          " ; allowed " + ", ".join(f"{R.MARGIN * b:.3e}" for b in bounds))
    for name, e, b in zip("pmv", errs, bounds):
        assert e <= R.MARGIN * b, (case.key, what, name, e, R.MARGIN * b)
    if case.cdt is not None:   # the 16-bit copy is the fp32 master rounded once
        for c, p in zip(got["copy"], got["p"]):
            assert torch.equal(c, p.to(case.cdt))
    if case.op == "lamb":
        print("   norm", got["norm"], "ref", ref["norm"])
        assert got["norm"] == pytest.approx(ref["norm"], rel=R.NORM_RTOL)


def _case_layouts(cases):
    out = []
    for c in cases:
        places = ["aligned"] if c.sizes == "many" else ["aligned", "unaligned"]
        if c.sizes == "default" and c.cdt is not None and c.gdt != F32:
            places.append("mixed")
        out += [pytest.param(c.key, pl, id=f"{c.name}-{pl}") for pl in places]
    return out


@pytest.mark.parametrize("key,place", _case_layouts(R.SGD_CASES + R.ADAM_CASES + R.LAMB_CASES))
def test_optimizer_case_matches_reference(key, place):
    case = R.CASES[key]
    # the device gradient scale where the case has one and the layout is not the plain one (SGD,
    # Adam), always for LAMB's bench configuration
    scale_tensor = case.scale != 1.0 and (place != "aligned" or (case.op == "lamb" and case.cdt is not None))
    got = R.run_case(case, DEV, place=place, scale_tensor=scale_tensor)
    _check_plan(got["lists"], case.chunk, case.sizes, place)
    _assert_state(case, got, R.reference(key), place)


# ----------------------------------------------------------------------------
# the plan's own entry points: device step counter, device first-run flag, skip flag
# ----------------------------------------------------------------------------
def _run_plan(case, *, place="aligned", scale_tensor=False, skip_first=False):
    """NSTEPS steps of `case` through MTPlan.sgd / adam / lamb with the device-side counters
    (Adam's and LAMB's step, SGD's first-run flag) and a skip flag. skip_first: one more call in
    front with the skip flag raised, which must leave every tensor and counter bit-for-bit alone."""
    get_plan, _ = _ops()
    h = case.h
    grads_c, g, p, m, v, cp, lists = R.setup_case(case, DEV, place)
    plan = get_plan(lists, case.chunk)
    noop, step_t, first = _flag(0), _flag(0), _flag(1)
    sc_t = torch.tensor([case.scale], device=DEV) if scale_tensor else None
    sc_f = 1.0 if scale_tensor else case.scale
    norm = None

    def call(k):
        if case.op == "sgd":
            plan.sgd(h["lr"], h["momentum"], h["dampening"], h["wd"], h["nesterov"], False,
                     h["wd_after_momentum"], sc_f, sc_t, noop, first)
        elif case.op == "adam":
            plan.adam(h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], 1.0, 1.0, h["adamw"], sc_f, sc_t,
                      noop, step_t, h["bias_correction"])
        else:
            gn = torch.tensor([R.lamb_supplied_norm(case, grads_c[k])], device=DEV) \
                if h["supplied_norm"] else None
            return float(plan.lamb(h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], h["max_grad_norm"],
                                   h["adamw"], h["bias_correction"], h["grad_averaging"], h["use_nvlamb"],
                                   sc_f, sc_t, noop, None, step_t, gn)[0])

    if skip_first:
        state = [t for lst in lists[1:] for t in lst] + [step_t, first]
        before = [t.clone() for t in state]
        noop.fill_(1)
        call(0)
        for a, b in zip(state, before):
            assert torch.equal(a, b), "a skipped step changed state"
        assert int(step_t) == 0 and int(first) == 1 and int(noop) == 1
        noop.zero_()
    for k in range(R.NSTEPS):
        for dst, src in zip(g, grads_c[k]):
            dst.copy_(src)
        norm = call(k)
    if case.op == "sgd":
        assert int(first) == 0
    else:
        assert int(step_t) == R.NSTEPS
    return {"p": p, "m": m, "v": [] if case.op == "sgd" else v, "copy": cp, "norm": norm, "lists": lists}


@pytest.mark.parametrize("key", [c.key for c in R.ADAM_CASES])
def test_adam_device_step_counter(key):
    """Bias corrections from the device counter (powf) instead of the host's."""
    case = R.CASES[key]
    _assert_state(case, _run_plan(case), R.reference(key), "device step")


@pytest.mark.parametrize("key", ["sgd/mom-damp-wd-f32", "sgd/nest-wdafter-bf16-cbf16"])
def test_sgd_device_first_run_flag(key):
    """first_run comes from the device flag: step 0 initialises the momentum buffer, 1 and 2 do not."""
    case = R.CASES[key]
    _assert_state(case, _run_plan(case), R.reference(key), "device first-run flag")


@pytest.mark.parametrize("key", ["adam/adamw-bf16-cbf16", "adam/l2-bf16-cbf16", "sgd/nest-wdafter-bf16-cbf16"])
@pytest.mark.parametrize("place", ["aligned", "unaligned"])
def test_float_and_device_grad_scale_are_bit_identical(key, place):
    case = R.CASES[key]
    a = _run_plan(case, place=place, scale_tensor=False)
    b = _run_plan(case, place=place, scale_tensor=True)
    for k in ("p", "m", "v", "copy"):
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x, y), k


@pytest.mark.parametrize("key", ["sgd/mom-damp-wdafter-bf16-cbf16-many", "sgd/mom-wd-f16-cf16",
                                 "adam/adamw-bf16-cbf16", "adam/adamw-bf16-cbf16-many",
                                 "lamb/bench-wd-adamw-clip", "lamb/bench-wd-l2-noavg-gnorm-many"])
def test_skipped_step_changes_nothing_and_uses_up_nothing(key):
    """Skip flag raised: p, m, v / momentum, copy and the device counters stay bit-for-bit. The
    next step is then the reference's step 1 (momentum initialised, bias corrections of step 1)."""
    case = R.CASES[key]
    got = _run_plan(case, scale_tensor=True, skip_first=True)
    _assert_state(case, got, R.reference(key), "after a skipped step")


# ----------------------------------------------------------------------------
# FusedLAMB (fused-master mode as amp O2 sets it up, and plain fp32)
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["lamb/bench-wd-adamw-clip", "lamb/f32-wd0-adamw-noclip",
                                 "lamb/f32-wd-l2-noavg-noclip"])
def test_fused_lamb_optimizer_matches_reference(key):
    from apex.optimizers import FusedLAMB

    case = R.CASES[key]
    h = case.h
    ps_c, grads_c = R.case_inputs(case)
    masters = [torch.nn.Parameter(p.to(DEV)) for p in ps_c]
    opt = FusedLAMB(masters, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"],
                    adam_w_mode=h["adamw"], grad_averaging=h["grad_averaging"],
                    max_grad_norm=h["max_grad_norm"], use_nvlamb=h["use_nvlamb"])
    owners = masters
    if case.cdt is not None:   # what amp.initialize(opt_level="O2") attaches
        owners = [torch.nn.Parameter(p.to(DEV).to(case.cdt)) for p in ps_c]
        opt._amp_model_params = [owners]
        opt._amp_grad_scale = torch.tensor([case.scale], device=DEV)
        opt._amp_noop = _flag()
    else:
        assert case.scale == 1.0
    for k in range(R.NSTEPS):
        for o, gk in zip(owners, grads_c[k]):
            o.grad = gk.to(DEV)
        opt.step()
    if case.cdt is not None:
        assert int(opt._amp_noop) == 0
    got = {"p": [x.detach() for x in masters], "m": [opt.state[x]["exp_avg"] for x in masters],
           "v": [opt.state[x]["exp_avg_sq"] for x in masters],
           "copy": [o.detach() for o in owners] if case.cdt is not None else None,
           "norm": float(opt._gnorm)}
    _assert_state(case, got, R.reference(key), "FusedLAMB")
    assert opt.state_dict()["param_groups"][0]["step"] == R.NSTEPS


# ----------------------------------------------------------------------------
# LARC
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("gdt,pdt", [(F32, F32), (BF16, BF16)], ids=["f32", "bf16"])
@pytest.mark.parametrize("clip,wd", R.LARC_CASES)
def test_larc_matches_reference(clip, wd, gdt, pdt):
    from apex.parallel.LARC import LARC

    hp = R.LARC_HP
    gs_c, ps_c = R.larc_inputs(gdt, pdt)
    params = [torch.nn.Parameter(p.to(DEV)) for p in ps_c]
    for x, g in zip(params, gs_c):
        x.grad = g.to(DEV)
    sgd = torch.optim.SGD(params, lr=hp["lr"], weight_decay=wd)
    LARC(sgd, trust_coefficient=hp["trust"], clip=clip, eps=hp["eps"]).step()
    assert sgd.param_groups[0]["weight_decay"] == wd   # restored after the step
    grads = [x.grad for x in params]
    ref_g = R.ref_larc_grads(gs_c, ps_c, wd=wd, clip=clip, **hp)
    ref_p = [p.double() - hp["lr"] * g for p, g in zip(ps_c, ref_g)]
    for i in (R.LARC_ZERO_GRAD, R.LARC_ZERO_PARAM):
        assert torch.equal(grads[i].cpu(), gs_c[i])   # a zero norm leaves the gradient alone
    assert torch.equal(params[R.LARC_ZERO_GRAD].detach().cpu(), ps_c[R.LARC_ZERO_GRAD])
    if gdt == F32:
        eg, ep = R.max_abs_err(grads, ref_g), R.max_abs_err(params, ref_p)
        bg, bp = R.LARC_BOUNDS[(clip, wd != 0)]
        print(f"larc: |err| grad {eg:.3e} (allowed {R.MARGIN * bg:.3e}) param {ep:.3e} (allowed {R.MARGIN * bp:.3e})")
        assert eg <= R.MARGIN * bg and ep <= R.MARGIN * bp
    else:
        # the fp32 value before the rounding carries the two fp32 norms, each within 8e-6 relative
        # (NORM_RTOL's derivation); the stepped parameter adds lr times the gradient's error to
        # its own rounding and to the fp32 evaluation of p - lr*g
        eg = R.ulp_excess(grads, ref_g, gdt, [2 * 8e-6 * g.abs() for g in ref_g])
        ep = R.ulp_excess(params, ref_p, pdt,
                          [hp["lr"] * (R.HALF_ULP[gdt] + 2 * 8e-6) * g.abs() + R.TINY[gdt] +
                           2.0 ** -23 * (p.double().abs() + hp["lr"] * g.abs()) for g, p in zip(ref_g, ps_c)])
        print("larc bf16: error / one rounding: grad", eg, "param", ep)
        assert eg <= 1.0 and ep <= 1.0


# ----------------------------------------------------------------------------
# plan reuse
# ----------------------------------------------------------------------------
def test_plan_does_not_match_resized_or_reinterpreted_tensors():
    get_plan, _ = _ops()
    n = 5000
    x, y = torch.randn(n, device=DEV), torch.zeros(n, device=DEV)
    plan = get_plan([[x], [y]], R.DEFAULT_CHUNK)
    assert plan.matches([[x], [y]])
    xb = x.view(BF16)[:n]   # same pointer, same numel, other dtype
    assert xb.data_ptr() == x.data_ptr() and xb.numel() == n
    assert not plan.matches([[xb], [y]])
    ptrs = (x.data_ptr(), y.data_ptr())
    x.resize_(n // 2)
    y.resize_(n // 2)
    assert (x.data_ptr(), y.data_ptr()) == ptrs
    assert not plan.matches([[x], [y]])


def test_scale_after_resize_writes_only_the_new_extent():
    _, ops = _ops()
    n = 5000
    x, y = torch.randn(n, device=DEV), torch.zeros(n, device=DEV)
    yfull = y.as_strided((n,), (1,))   # the storage stays allocated at n elements after the resize
    x0 = x.clone()
    ops.multi_tensor_scale(R.DEFAULT_CHUNK, None, [[x], [y]], 2.0)
    assert torch.equal(yfull, x0 * 2.0)
    x.resize_(n // 2)
    y.resize_(n // 2)
    yfull.fill_(-7.0)
    ops.multi_tensor_scale(R.DEFAULT_CHUNK, None, [[x], [y]], 4.0)   # same ids, same pointers
    assert torch.equal(yfull[:n // 2], x0[:n // 2] * 4.0)
    assert bool((yfull[n // 2:] == -7.0).all()), "scale wrote past the resized tensor"


# ----------------------------------------------------------------------------
# FusedAdam's legacy clip with amp's gradient scale attached
# ----------------------------------------------------------------------------
def test_fused_adam_legacy_clip_applies_with_amp_grad_scale():
    """step(grads=, scale=, grad_norms=) with max_grad_norm folds 1/scale and the clip into a host
    factor; amp's device scale must multiply it, not replace it."""
    from apex.optimizers import FusedAdam

    case = R.CASES["adam/adamw-f32-clipamp"]
    h, c = case.h, R.ADAM_CLIP_AMP
    ps_c, grads_c = R.case_inputs(case)
    params = [torch.nn.Parameter(p.to(DEV)) for p in ps_c]
    opt = FusedAdam(params, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], adam_w_mode=True,
                    weight_decay=h["wd"], max_grad_norm=c["max_grad_norm"])
    opt._amp_grad_scale = torch.tensor([c["amp_scale"]], device=DEV)
    g = [t.to(DEV) for t in grads_c[0]]
    for k in range(R.NSTEPS):
        for dst, src in zip(g, grads_c[k]):
            dst.copy_(src)
        opt.step(grads=g, scale=c["scale"], grad_norms=c["norm"])
    got = {"p": [x.detach() for x in params], "m": [opt.state[x]["exp_avg"] for x in params],
           "v": [opt.state[x]["exp_avg_sq"] for x in params], "copy": None}
    _assert_state(case, got, R.reference(case.key), "FusedAdam clip under amp")
