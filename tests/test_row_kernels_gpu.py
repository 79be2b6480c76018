"""The row kernels (csrc/softmax.hip, csrc/xentropy.hip, csrc/layer_norm.hip) against the float64
reference of tests/row_reference.py, on every dispatch path.

Rows are kept tiny: these kernels go wrong along the column and dispatch axes. Softmax: every KPL
and both sides of each boundary, row counts that leave a block ragged and one that fills it, the
three mask modes, -inf inputs, fp32 through the binding, and the calls FusedScaleMaskSoftmax has
to send to the PyTorch formulation. Cross-entropy: the 16-byte and the scalar path, the second
sweep of a thread (V > 2048), ignored and out-of-range labels, the three ways a loss gradient
arrives, -inf padding, shifted logits. LayerNorm / RMSNorm: fast VPT 1 / 2 / 4, forward 8, wide
5 .. 8, the slow path, every (activation, weight) dtype pair, and no affine parameters at all.

Every output is held to row_reference.check (one rounding to the output dtype plus C = 2**-16 of
the output's cond); lse, loss, mean and rstd to MARGIN times the measured error of the fp32 CPU
formulation plus 2**-20 * max(1, |ref|); what the contract makes exact is compared with ==. Every
test prints its figures before asserting; the worst per kernel and dtype are printed at the end.
"""
import pytest
import torch

import row_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F16, BF16 = R.F32, R.F16, R.BF16
SMX_MODE_CODE = {"none": 0, "mask": 1, "causal": 2}


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    R.WORST.clear()
    yield
    print("\nworst |got - ref| / bound per output and dtype:")
    for tag in sorted(R.WORST):
        print(f"  {tag}: {R.WORST[tag][0]:.3f}  ({R.WORST[tag][1]})")


def _C():
    import apex

    return apex._ext.require()


def _check(got, ref, cond, dtype, what, out):
    return R.check(got, ref, cond, dtype, what, tag=f"{out} {R.DT_NAME[dtype]}")


def _scalar(got, ref, bound, what, out):
    assert got.dtype == F32
    ex = R.scalar_excess(got, ref, bound)
    tag = f"{out} (scalar)"
    if ex > R.WORST.get(tag, (-1.0, ""))[0]:
        R.WORST[tag] = (ex, what)
    print(f"{what} {out}: error / allowance = {ex:.3f} (recorded fp32 CPU error {bound:.3e})")
    assert ex <= 1.0, (what, out, ex)
    return ex


# ----------------------------------------------------------------------------
# softmax
# ----------------------------------------------------------------------------
def mask_func(s, m):
    return s.masked_fill(m.bool(), -10000.0)


def _run_softmax(case, x, dy, mask):
    """(y, dx) of the kernels: 16-bit through the autograd functions, fp32 through the binding."""
    from apex.transformer.functional import fused_softmax as fs

    xd, dyd = x.to(DEV), dy.to(DEV)
    md = mask.to(DEV) if mask is not None else None
    if case.dtype == F32:
        C = _C()
        y = C.scaled_masked_softmax_fwd(xd, md, case.scale, SMX_MODE_CODE[case.kernel_mode], case.h)
        return y, C.scaled_masked_softmax_bwd(dyd, y, case.scale)
    xd.requires_grad_(True)
    if case.kernel_mode == "mask":
        y = fs.ScaledMaskedSoftmax.apply(xd, md, case.scale)
    elif case.kernel_mode == "causal":
        y = fs.ScaledUpperTriangMaskedSoftmax.apply(xd, case.scale)
    else:
        y = fs.ScaledSoftmax.apply(xd, case.scale)
    y.backward(dyd)
    return y.detach(), xd.grad


def _assert_softmax(case, x, dy, mask, y, dx):
    name = case.name
    assert y.dtype == case.dtype and dx.dtype == case.dtype
    ref, cond = R.ref_softmax_fwd(x, case.scale, case.kernel_mode, mask)
    y_c, dx_c = y.cpu(), dx.cpu()
    rdx, cdx = R.ref_softmax_bwd(dy, y_c, case.scale)
    fw = R.ratio(y_c, ref, cond, case.dtype)[0]
    bw = R.ratio(dx_c, rdx, cdx, case.dtype)[0]
    print(f"{name}: y {fw:.3f} dx {bw:.3f} of the bound")
    _check(y_c, ref, cond, case.dtype, name + " y", "softmax y")
    _check(dx_c, rdx, cdx, case.dtype, name + " dx", "softmax dx")
    if case.kernel_mode == "causal":
        dead = torch.ones(case.sq, case.sk).triu(1).bool().expand(ref.shape)
        assert bool((y_c[dead] == 0).all()) and bool((dx_c[dead] == 0).all())
        assert bool((y_c[..., 0, 0] == 1).all())
    if case.neginf:
        gone = x == -R.INF
        assert bool((y_c[gone] == 0).all()) and bool((dx_c[gone] == 0).all())
    if case.mode == "maskh":
        assert bool((ref[-1, -1, -1] == 1.0 / case.sk).all())


@pytest.mark.parametrize("name", list(R.SMX_CASES))
def test_softmax_matches_reference(name):
    case = R.SMX_CASES[name]
    assert _C().scaled_softmax_supported(case.sk)
    assert ((case.b * case.h * case.sq) % 4 == 0) == ("rows4k" in name)   # ragged last block, or none
    x, dy, mask = R.smx_inputs(case)
    y, dx = _run_softmax(case, x, dy, mask)
    _assert_softmax(case, x, dy, mask, y, dx)


def _module(dt, causal, scale):
    from apex.transformer.enums import AttnMaskType
    from apex.transformer.functional import FusedScaleMaskSoftmax

    mt = AttnMaskType.causal if causal else AttnMaskType.padding
    return FusedScaleMaskSoftmax(dt == F16, dt == BF16, mt, True, mask_func, True, scale)


def _spy(mod, monkeypatch):
    """Which of the module's two paths ran."""
    ran = []
    fused, eager = mod.forward_fused_softmax, mod.forward_torch_softmax
    monkeypatch.setattr(mod, "forward_fused_softmax", lambda i, m: (ran.append("fused"), fused(i, m))[1])
    monkeypatch.setattr(mod, "forward_torch_softmax", lambda i, m: (ran.append("torch"), eager(i, m))[1])
    return ran


@pytest.mark.parametrize("dt", [F16, BF16], ids=R.DT_NAME.get)
def test_softmax_module_causal_square(dt, monkeypatch):
    """sq == sk == 520 through the module: the fused causal kernel, KPL 2 with a part-filled pack row."""
    case = R.SmxCase(f"smx/{R.DT_NAME[dt]}-causal-sk520-sq520-module", dt, 1, 1, 520, 520, R.f32(0.125), "causal")
    x, dy, _ = R.smx_inputs(case)
    mod = _module(dt, True, case.scale)
    ran = _spy(mod, monkeypatch)
    xd = x.to(DEV).requires_grad_(True)
    y = mod(xd, None)
    y.backward(dy.to(DEV))
    assert ran == ["fused"]
    _assert_softmax(case, x, dy, None, y.detach(), xd.grad)


@pytest.mark.parametrize("dt", [F16, BF16], ids=R.DT_NAME.get)
@pytest.mark.parametrize("kind", ["mask-b-1-sq-sk", "mask-b-h-sq-sk", "mask-1-1-sq-sk", "mask-b-1-1-sk",
                                  "offset-input", "offset-dy"])
def test_softmax_module_dispatch(dt, kind, monkeypatch):
    """The masks and inputs the kernels take run fused; a broadcast mask batch, a broadcast query
    dimension and an input off 16-byte alignment go to the PyTorch formulation, and neither
    raises. Each against the float64 reference."""
    b, h, sq, sk = 2, 3, 7, 520
    case = R.SmxCase(f"smx/{R.DT_NAME[dt]}-module-{kind}", dt, b, h, sq, sk, R.f32(0.125),
                     "none" if kind.startswith("offset") else "mask")
    g = R._gen(case.name)
    x = (torch.randn((b, h, sq, sk), generator=g) * 4).to(dt)
    dy = torch.randn((b, h, sq, sk), generator=g).to(dt)
    mshape = {"mask-b-1-sq-sk": (b, 1, sq, sk), "mask-b-h-sq-sk": (b, h, sq, sk), "mask-1-1-sq-sk": (1, 1, sq, sk),
              "mask-b-1-1-sk": (b, 1, 1, sk)}.get(kind)
    mask = (torch.rand(mshape, generator=g) < 0.3) if mshape else None
    mod = _module(dt, False, case.scale)
    ran = _spy(mod, monkeypatch)
    if kind == "offset-input":
        buf = torch.zeros(x.numel() + 1, dtype=dt, device=DEV)
        buf[1:] = x.to(DEV).reshape(-1)
        xd = buf[1:].view(b, h, sq, sk)
        assert xd.is_contiguous() and xd.data_ptr() % 16 != 0
    else:
        xd = x.to(DEV)
    xd = xd.detach().requires_grad_(True)
    y = mod(xd, mask.to(DEV) if mask is not None else None)
    want = "torch" if kind in ("mask-1-1-sq-sk", "mask-b-1-1-sk", "offset-input") else "fused"
    assert ran == [want], (kind, ran)
    assert y.dtype == dt
    ref, cond = R.ref_softmax_fwd(x, case.scale, case.mode, mask)
    _check(y.detach().cpu(), ref, cond, dt, case.name + " y", f"softmax y via {want} path")
    if want == "torch":
        return
    dyd = dy.to(DEV)
    if kind == "offset-dy":
        buf = torch.zeros(dy.numel() + 1, dtype=dt, device=DEV)
        buf[1:] = dyd.reshape(-1)
        dyd = buf[1:].view(b, h, sq, sk)
        assert dyd.data_ptr() % 16 != 0
    y.backward(dyd)
    rdx, cdx = R.ref_softmax_bwd(dy, y.detach().cpu(), case.scale)
    _check(xd.grad.cpu(), rdx, cdx, dt, case.name + " dx", "softmax dx")


def test_softmax_binding_rejects_what_the_kernel_cannot_index():
    C = _C()
    b, h, sq, sk = 2, 3, 4, 64
    x = torch.zeros(b, h, sq, sk, dtype=F16, device=DEV)

    def m(*shape):
        return torch.zeros(shape, dtype=torch.uint8, device=DEV)

    for bad in (m(1, 1, sq, sk), m(b, 2, sq, sk), m(b, 1, 1, sk), m(b * sq, sk), m(b, 1, sq, sk + 8)):
        with pytest.raises(RuntimeError, match="mask"):
            C.scaled_masked_softmax_fwd(x, bad, 1.0, 1, h)
    with pytest.raises(RuntimeError, match="heads"):
        C.scaled_masked_softmax_fwd(x, m(b, 1, sq, sk), 1.0, 1, h + 1)
    off = torch.zeros(x.numel() + 1, dtype=F16, device=DEV)[1:].view(b, h, sq, sk)
    with pytest.raises(RuntimeError, match="aligned"):
        C.scaled_masked_softmax_fwd(off, None, 1.0, 0, h)
    with pytest.raises(RuntimeError, match="aligned"):
        C.scaled_masked_softmax_bwd(off, x, 1.0)
    moff = torch.zeros(b * sq * sk + 1, dtype=torch.uint8, device=DEV)[1:].view(b, 1, sq, sk)
    with pytest.raises(RuntimeError, match="aligned"):
        C.scaled_masked_softmax_fwd(x, moff, 1.0, 1, h)


# ----------------------------------------------------------------------------
# cross-entropy
# ----------------------------------------------------------------------------
DLOSS_MODES = ["vector", "sum", "mean"]


def _run_xent(case, x, labels, dloss, mode, offset=False):
    """(lse, loss, dlogits, per-row loss gradient used) of the kernels."""
    from apex.contrib.xentropy import SoftmaxCrossEntropyLoss
    from apex.contrib.xentropy.softmax_xentropy import softmax_xentropy

    C = _C()
    N, V = x.shape
    if offset:
        buf = torch.zeros(N * V + 1, dtype=x.dtype, device=DEV)
        buf[1:] = x.to(DEV).reshape(-1)
        xd = buf[1:].view(N, V)
        assert xd.is_contiguous() and xd.data_ptr() % 16 != 0
    else:
        xd = x.to(DEV)
    xd = xd.detach().requires_grad_(True)
    ld = labels.to(DEV)
    _, lse = C.xent_fwd(xd.detach(), ld, case.smoothing, case.ignore_index)
    if mode == "mean":
        total = softmax_xentropy(xd, ld, case.smoothing, case.ignore_index, reduction="mean")
        total.backward()
        count = max(int((labels != case.ignore_index).sum()), 1)
        g = torch.full((N,), R.f32(1.0 / count))
        loss = SoftmaxCrossEntropyLoss.apply(xd.detach(), ld, case.smoothing, case.ignore_index, False)
        return lse, loss, xd.grad, g, total.detach()
    loss = SoftmaxCrossEntropyLoss.apply(xd, ld, case.smoothing, case.ignore_index, False)
    if mode == "sum":
        loss.sum().backward()   # the gradient arrives with stride 0
        g = torch.ones(N)
    else:
        loss.backward(dloss.to(DEV))
        g = dloss
    return lse, loss.detach(), xd.grad, g, None


def _assert_xent(case, x, labels, got, *, grads=True):
    lse, loss, dx, g, total = got
    name = case.name
    ref = R.ref_xent(x, labels, case.smoothing, case.ignore_index, g)
    dead = ~ref["valid"]
    assert int(dead.sum()) >= 3
    loss_c, dx_c = loss.cpu(), dx.cpu()
    assert dx_c.dtype == case.dtype
    _scalar(lse.cpu(), ref["lse"], R.BOUNDS[name][0], name, "xent lse")
    _scalar(loss_c, ref["loss"], R.BOUNDS[name][1], name, "xent loss")
    assert bool((loss_c[dead] == 0).all()) and bool((dx_c[dead] == 0).all())
    if total is not None:
        count = max(int((labels != case.ignore_index).sum()), 1)
        want = float(ref["loss"].sum()) / count
        # the rows' allowances add up; the fp32 sum of 7 rows and the divide add 8 roundings
        tol = float((R.MARGIN * R.BOUNDS[name][1] + R.SCALAR_FAST * ref["loss"].abs().clamp(min=1.0)).sum()) / count
        print(f"{name}: mean loss off by {abs(float(total) - want):.3e}, allowed {tol + 2.0 ** -21 * abs(want):.3e}")
        assert abs(float(total) - want) <= tol + 2.0 ** -21 * abs(want)
    if grads:
        w = R.ratio(dx_c, ref["dlogits"], ref["dlogits_cond"], case.dtype)[0]
        print(f"{name}: dlogits {w:.3f} of the bound")
        _check(dx_c, ref["dlogits"], ref["dlogits_cond"], case.dtype, name + " dlogits", "xent dlogits")
    else:
        assert bool(torch.isfinite(dx_c.float()).all())
    return ref


PLAIN_XENT = [n for n, c in R.XENT_CASES.items() if c.kind == "plain"]


@pytest.mark.parametrize("name", PLAIN_XENT)
def test_xentropy_matches_reference(name):
    case = R.XENT_CASES[name]
    x, labels, dloss = R.xent_inputs(case)
    mode = DLOSS_MODES[PLAIN_XENT.index(name) % 3]
    _assert_xent(case, x, labels, _run_xent(case, x, labels, dloss, mode))


@pytest.mark.parametrize("mode", DLOSS_MODES)
@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_NAME.get)
@pytest.mark.parametrize("V", [1000, 2056])
def test_xentropy_loss_gradient_forms(V, dt, mode):
    """An explicit vector, .sum().backward() (stride 0) and the mean reduction, on both paths."""
    case = next(c for c in R.XENT_CASES.values() if c.dtype == dt and c.V == V and c.smoothing > 0
                and c.kind == "plain" and not c.seed)
    x, labels, dloss = R.xent_inputs(case)
    _assert_xent(case, x, labels, _run_xent(case, x, labels, dloss, mode))


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_NAME.get)
@pytest.mark.parametrize("V", [8, 2048, 50304])
def test_xentropy_offset_view_takes_the_scalar_path(V, dt):
    """V % 8 == 0 but the logits start one element off 16-byte alignment."""
    case = next(c for c in R.XENT_CASES.values() if c.dtype == dt and c.V == V and c.smoothing > 0
                and c.kind == "plain")
    x, labels, dloss = R.xent_inputs(case)
    _assert_xent(case, x, labels, _run_xent(case, x, labels, dloss, "vector", offset=True))


@pytest.mark.parametrize("offset", [False, True], ids=["vector", "scalar"])
@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_NAME.get)
def test_xentropy_masked_vocabulary_padding(dt, offset):
    """V = 50304 with columns >= 50257 at -inf: whole 16-byte groups of -inf in a thread's second
    sweep. The loss is finite and the padding gets exact zeros."""
    case = R.XENT_CASES[f"xent/{R.DT_NAME[dt]}-V50304-s0.0-ign-100-neginf"]
    x, labels, dloss = R.xent_inputs(case)
    got = _run_xent(case, x, labels, dloss, "vector", offset=offset)
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    _assert_xent(case, x, labels, got)
    assert bool((got[2].cpu()[:, R.XENT_PAD_FROM:] == 0).all())


@pytest.mark.parametrize("name", [n for n, c in R.XENT_CASES.items() if c.kind == "shift"])
def test_xentropy_shift_invariance(name):
    """x and x + 1000 in fp32: each loss within its bound of its own reference, and so of each other
    up to what rounding x + 1000 to fp32 changes (the references differ by that)."""
    out = {}
    for n in (name.replace("-shift", "-plain"), name):
        case = R.XENT_CASES[n]
        x, labels, dloss = R.xent_inputs(case)
        got = _run_xent(case, x, labels, dloss, "vector")
        ref = _assert_xent(case, x, labels, got, grads=(case.kind == "plain"))
        out[case.kind] = (got[1].cpu().double(), ref["loss"])
    moved = (out["shift"][0] - out["plain"][0]).abs().max()
    ref_moved = (out["shift"][1] - out["plain"][1]).abs().max()
    print(f"{name}: losses moved by {float(moved):.3e}, the references by {float(ref_moved):.3e}")


def test_xentropy_fp16_logits_near_the_end_of_the_range():
    case = R.XENT_CASES["xent/f16-V2056-s0.1-ign-100-big"]
    x, labels, dloss = R.xent_inputs(case)
    assert float(x.float().abs().min()) > 59000
    got = _run_xent(case, x, labels, dloss, "vector")
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    _assert_xent(case, x, labels, got, grads=False)


def test_vocab_parallel_cross_entropy_tp1_route(monkeypatch):
    from apex.transformer import parallel_state as ps
    from apex.transformer.tensor_parallel.cross_entropy import vocab_parallel_cross_entropy

    monkeypatch.setattr(ps, "_MPU_TENSOR_MODEL_PARALLEL_WORLD_SIZE", 1)
    V, s = 2056, 0.1
    case = R.XentCase("xent/bf16-V2056-tp1", BF16, V, R.f32(s * V / (V - 1)), -100)
    x, labels, dloss = R.xent_inputs(case)
    xd = x.to(DEV).view(1, R.XENT_N, V).requires_grad_(True)
    loss = vocab_parallel_cross_entropy(xd, labels.to(DEV).view(1, R.XENT_N), s)
    assert loss.shape == (1, R.XENT_N) and loss.dtype == F32
    loss.backward(dloss.to(DEV).view(1, R.XENT_N))
    # the route hands s V / (V - 1) to the kernel as a double; the kernel rounds it to fp32
    ref = R.ref_xent(x, labels, case.smoothing, -100, dloss)
    twin = next(n for n, c in R.XENT_CASES.items() if c.dtype == BF16 and c.V == V and c.smoothing > 0)
    bound = R.BOUNDS[twin][1]   # the table's bf16 case of this V with smoothing: other draws, the same arithmetic
    _scalar(loss.view(-1).cpu(), ref["loss"], bound, case.name, "xent loss")
    assert xd.grad.dtype == BF16
    _check(xd.grad.view(R.XENT_N, V).cpu(), ref["dlogits"], ref["dlogits_cond"], BF16, case.name + " dlogits",
           "xent dlogits")


# ----------------------------------------------------------------------------
# LayerNorm / RMSNorm
# ----------------------------------------------------------------------------
def _offset_view(t):
    """The same values one element off 16-byte alignment: a view into a flat buffer."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:] = t.to(DEV).reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _run_norm(case, x, gamma, beta, dy, *, route="functional", offset_weight=False, shape=None):
    """dict(y, dx, dgamma, dbeta, mean, rstd) of the kernels. route "functional": the autograd
    function behind fused_*_norm(_affine); "module": (Mixed)Fused*Norm modules."""
    from apex import normalization as N
    from apex.normalization.fused_layer_norm import (fused_layer_norm, fused_layer_norm_affine, fused_rms_norm,
                                                     fused_rms_norm_affine)

    C = _C()
    nshape = tuple(shape) if shape else (case.cols,)
    xd = x.to(DEV)
    if shape:
        xd = xd.view(case.rows, *nshape)
    xd = xd.requires_grad_(True)
    dyd = dy.to(DEV).view(xd.shape)
    w = b = None
    if gamma is not None:
        w = (_offset_view(gamma) if offset_weight else gamma.to(DEV)).view(nshape).detach().requires_grad_(True)
        assert (w.data_ptr() % 16 != 0) == offset_weight
    if beta is not None:
        b = (_offset_view(beta) if offset_weight else beta.to(DEV)).view(nshape).detach().requires_grad_(True)
    if route == "module":
        mixed = case.wdt != case.xdt
        cls = {(False, False): N.FusedLayerNorm, (False, True): N.MixedFusedLayerNorm,
               (True, False): N.FusedRMSNorm, (True, True): N.MixedFusedRMSNorm}[(case.rms, mixed)]
        mod = cls(nshape, eps=case.eps, elementwise_affine=case.affine).to(DEV)
        if case.affine:
            mod = mod.to(case.xdt)     # the Mixed modules keep their parameters fp32
            assert mod.weight.dtype == case.wdt
            with torch.no_grad():
                mod.weight.copy_(w)
                if b is not None:
                    mod.bias.copy_(b)
        y = mod(xd)
        y.backward(dyd)
        dg = mod.weight.grad if case.affine else None
        db = mod.bias.grad if (case.affine and not case.rms) else None
    else:
        if case.rms:
            y = fused_rms_norm_affine(xd, w, nshape, case.eps) if case.affine else \
                fused_rms_norm(xd, nshape, case.eps)
        else:
            y = fused_layer_norm_affine(xd, w, b, nshape, case.eps) if case.affine else \
                fused_layer_norm(xd, nshape, case.eps)
        y.backward(dyd)
        dg = w.grad if w is not None else None
        db = b.grad if b is not None else None
    _, mean, rstd = C.ln_fwd(xd.detach(), case.cols, w.detach() if w is not None else None,
                             b.detach() if b is not None else None, case.eps, case.rms)
    return {"y": y.detach(), "dx": xd.grad, "dgamma": dg, "dbeta": db, "mean": mean, "rstd": rstd}


def _assert_norm(case, got, ref=None):
    name = case.name
    ref = ref or R.norm_reference(name)
    kind = "rmsnorm" if case.rms else "layernorm"
    rc = (case.rows, case.cols)
    assert got["y"].dtype == case.xdt and got["dx"].dtype == case.xdt
    if not case.rms:
        _scalar(got["mean"].cpu(), ref["mean"], R.BOUNDS[case.stats][0], name, f"{kind} mean")
    else:
        assert got["mean"].numel() == 0
    _scalar(got["rstd"].cpu(), ref["rstd"], R.BOUNDS[case.stats][1], name, f"{kind} rstd")
    outs = [("y", case.xdt, rc), ("dx", case.xdt, rc)]
    if case.affine:
        outs.append(("dgamma", case.wdt, (case.cols,)))
        if not case.rms:
            outs.append(("dbeta", case.wdt, (case.cols,)))
    else:
        assert got["dgamma"] is None and got["dbeta"] is None
    vals = {k: got[k].detach().cpu().reshape(shape) for k, _, shape in outs}
    for k, dt, _ in outs:
        assert vals[k].dtype == dt, (k, vals[k].dtype)
    print(name + ":", " ".join(f"{k} {R.ratio(vals[k], ref[k], ref[k + '_cond'], dt)[0]:.3f}" for k, dt, _ in outs),
          "of the bound")
    for k, dt, _ in outs:
        _check(vals[k], ref[k], ref[k + "_cond"], dt, f"{name} {k}", f"{kind} {k}")


@pytest.mark.parametrize("name", list(R.NORM_CASES))
def test_norm_matches_reference(name):
    """Equal dtype pairs through the functional forms, fp32 weights with 16-bit activations through
    the MixedFused* modules; the cases without affine parameters alternate between the two."""
    case = R.NORM_CASES[name]
    x, gamma, beta, dy = R.norm_inputs(case)
    if case.affine:
        route = "module" if case.wdt != case.xdt else "functional"
    else:
        route = ("functional", "module")[list(R.NORM_CASES).index(name) % 2]
    _assert_norm(case, _run_norm(case, x, gamma, beta, dy, route=route))


@pytest.mark.parametrize("name", ["ln/bf16-wbf16-r5-c512", "ln/bf16-wf32-r5-c520", "rms/f16-wf16-r5-c1032",
                                  "ln/f32-wf32-r5-c2560"])
def test_norm_misaligned_weight_takes_the_slow_path(name):
    """gamma / beta as views one element into a flat buffer, at column counts of the fast and wide
    paths: the 16-byte kernels cannot load them, the block-per-row kernels give the same numbers."""
    case = R.NORM_CASES[name]
    x, gamma, beta, dy = R.norm_inputs(case)
    _assert_norm(case, _run_norm(case, x, gamma, beta, dy, offset_weight=True))


@pytest.mark.parametrize("name", ["ln/f32-wf32-r5-c64", "rms/bf16-wbf16-r5-c64"])
def test_norm_two_dimensional_normalized_shape(name):
    """x [5, 4, 16] normalised over its last two dimensions, weight [4, 16]."""
    case = R.NORM_CASES[name]
    x, gamma, beta, dy = R.norm_inputs(case)
    _assert_norm(case, _run_norm(case, x, gamma, beta, dy, route="module", shape=(4, 16)))


@pytest.mark.parametrize("name", ["ln/bf16-wf32-r5-c520", "ln/f32-wf32-r5-c2560", "ln/bf16-wbf16-r5-c100"])
def test_norm_backward_into_given_destinations(name):
    """dgamma_out / dbeta_out of C.ln_bwd: slots of a larger buffer, which must be written and
    nothing beside them."""
    C = _C()
    case = R.NORM_CASES[name]
    x, gamma, beta, dy = R.norm_inputs(case)
    xd, w, b, dyd = x.to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(DEV)
    y, mean, rstd = C.ln_fwd(xd, case.cols, w, b, case.eps, False)
    bucket = torch.full((2 * case.cols + 24,), 7.0, dtype=case.wdt, device=DEV)
    dg_slot, db_slot = bucket[8:8 + case.cols], bucket[16 + case.cols:16 + 2 * case.cols]
    dx, dg, db = C.ln_bwd(dyd, xd, case.cols, w, b, mean, rstd, False, dg_slot, db_slot)
    assert dg.data_ptr() == dg_slot.data_ptr() and db.data_ptr() == db_slot.data_ptr()
    keep = torch.ones_like(bucket, dtype=torch.bool)
    keep[8:8 + case.cols] = False
    keep[16 + case.cols:16 + 2 * case.cols] = False
    assert bool((bucket[keep] == 7.0).all())
    _assert_norm(case, {"y": y, "dx": dx, "dgamma": dg_slot, "dbeta": db_slot, "mean": mean, "rstd": rstd})
    with pytest.raises(RuntimeError, match="beta without gamma"):
        C.ln_bwd(dyd, xd, case.cols, None, b, mean, rstd, False, None, None)
