"""The gated-activation HIP kernels (csrc/fused_ops.hip glu_fwd / glu_bwd) against the float64 reference of
glu_reference.py, through the autograd Function (apex.ops.fused.gated_act) and through the bindings.

Shapes are the smallest at which the column-chunk geometry can go wrong: F on both sides of the
256 x 8 block boundary and in a third block, rows around the 16-row floor of a row block, and one case
of more than 512 x 16 rows (rows per block > 16, last block ragged). Every case checks y, dgate, dup
and dbias by the bound, that x is left untouched, and that a second run gives the same bits."""
import pytest
import torch

import glu_reference as R
from glu_reference import ACT_GELU, ACT_GELU_TANH, ACT_SILU, ACTS, BF16, F16, F32, GLU_CASES

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    R.WORST.clear()
    yield
    print("\nworst |got - ref| / bound per output and dtype:")
    for tag in sorted(R.WORST):
        print(f"  {tag}: {R.WORST[tag][0]:.3f}  ({R.WORST[tag][1]})")


def _fops():
    from apex.ops import fused as fops

    return fops


def _C():
    from apex import _ext

    return _ext.require()


def _autograd(x, b, dy, act, fn=None):
    xr = x.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if b is not None else None
    y = fn(xr, br) if fn is not None else _fops().gated_act(xr, br, act)
    y.backward(dy)
    return y.detach(), xr.grad, (br.grad if br is not None else None)


@pytest.mark.parametrize("name", list(GLU_CASES))
def test_glu_case(name):
    case = GLU_CASES[name]
    x_c, b_c, dy_c = R.glu_inputs(case)
    x, dy = x_c.to(DEV), dy_c.to(DEV)
    b = b_c.to(DEV) if b_c is not None else None
    y, dx, db = _autograd(x, b, dy, case.act)
    assert y.shape == (case.rows, case.F) and dx.shape == x.shape and y.dtype == dx.dtype == case.xdt
    assert db is None or (db.shape == b.shape and db.dtype == case.bdt)
    assert torch.equal(x.cpu(), x_c), "x was modified"
    assert b is None or torch.equal(b.cpu(), b_c)
    ratios = R.check_all(case, y, dx, db, tagbase="glu")
    print(name + ":", " ".join(f"{k} {v:.3f}" for k, v in ratios.items()), "of the bound")
    # the bindings, which is also the second run: the same bits, dbias included
    C = _C()
    y2 = C.glu_fwd(x, b, case.act)
    dx2, db2 = C.glu_bwd(dy, x, b, case.act, b is not None)
    assert torch.equal(y2, y) and torch.equal(dx2, dx)
    assert (db2 is None) == (db is None) and (db is None or torch.equal(db2, db))
    assert torch.equal(x.cpu(), x_c), "x was modified"
    # no bias gradient asked for: dx the same, dbias skipped
    if b is not None:
        dx3, db3 = C.glu_bwd(dy, x, b, case.act, False)
        assert db3 is None and torch.equal(dx3, dx)


@pytest.mark.parametrize("dtype", [F16, BF16, F32])
@pytest.mark.parametrize("act", ACTS)
def test_extreme_gates(dtype, act):
    """Gates of +-30000 (fp16-representable): nothing overflows inside, y = v a up to its one rounding where
    the gate is positive and zero where it is negative, and every gradient is finite."""
    g = torch.Generator().manual_seed(5)
    rows, F_ = 17, 16
    sign = torch.where(torch.rand((rows, F_), generator=g) < 0.5, -1.0, 1.0)
    gate = (30000.0 * sign).to(dtype)
    assert bool((gate.double().abs() > 29000).all())
    up = ((torch.rand((rows, F_), generator=g) * 4 - 2)).to(dtype)
    dy = ((torch.rand((rows, F_), generator=g) * 4 - 2)).to(dtype)
    x = torch.cat([gate, up], 1).to(DEV)
    y, dx, _ = _autograd(x, None, dy.to(DEV), act)
    y, dx = y.cpu(), dx.cpu()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    pos = sign > 0
    want = (up.double() * gate.double()).to(dtype)
    assert torch.equal(y[pos], want[pos])
    assert bool((y[~pos] == 0).all())
    # act' is 1 / 0 and act is a / 0 there: dgate = dy v, dup = dy a, each rounded once; zero on the negative side
    assert torch.equal(dx[:, :F_][pos], (dy.double() * up.double()).to(dtype)[pos])
    assert torch.equal(dx[:, F_:][pos], (dy.double() * gate.double()).to(dtype)[pos])
    assert bool((dx[:, :F_][~pos] == 0).all()) and bool((dx[:, F_:][~pos] == 0).all())


def test_f_not_multiple_of_8_takes_reference_path():
    fops = _fops()
    g = torch.Generator().manual_seed(6)
    x = torch.randn((5, 200), generator=g).to(BF16).to(DEV)
    b = torch.randn((200,), generator=g).to(BF16).to(DEV)
    dy = torch.randn((5, 100), generator=g).to(BF16).to(DEV)
    got = _autograd(x, b, dy, ACT_SILU)
    want = _autograd(x, b, dy, ACT_SILU, fn=lambda x_, b_: fops.gated_act_reference(x_, b_, ACT_SILU))
    for a, w in zip(got, want):
        assert torch.equal(a, w)
    with pytest.raises(RuntimeError):   # the launcher itself declines
        _C().glu_fwd(x, b, ACT_SILU)


def test_zero_rows():
    fops = _fops()
    x = torch.empty((0, 32), dtype=BF16, device=DEV, requires_grad=True)
    b = torch.randn((32,), dtype=BF16, device=DEV, requires_grad=True)
    y = fops.gated_act(x, b, ACT_GELU_TANH)
    assert y.shape == (0, 16)
    y.sum().backward()
    assert x.grad.shape == (0, 32) and b.grad.shape == (32,) and not bool(b.grad.any())
    x3 = torch.empty((2, 0, 32), dtype=F32, device=DEV)
    assert fops.bias_swiglu(x3).shape == (2, 0, 16)


def test_bias_swiglu_3d_and_views():
    """[B, S, 2F] through bias_swiglu with gradients to x and the bias; a non-contiguous x and a bias
    that needs no gradient."""
    fops = _fops()
    g = torch.Generator().manual_seed(7)
    B, S, F_ = 2, 9, 24
    x_c = (torch.randn((B, S, 2 * F_), generator=g) * 4).to(BF16)
    b_c = torch.randn((2 * F_,), generator=g)   # fp32 bias, bf16 activations
    dy_c = torch.randn((B, S, F_), generator=g).to(BF16)
    x, b, dy = x_c.to(DEV), b_c.to(DEV), dy_c.to(DEV)
    y, dx, db = _autograd(x, b, dy, ACT_SILU, fn=lambda x_, b_: fops.bias_swiglu(x_, b_))
    assert y.shape == (B, S, F_) and dx.shape == (B, S, 2 * F_) and db.shape == (2 * F_,) and db.dtype == F32
    ref = R.ref_glu(x_c.reshape(-1, 2 * F_), b_c, dy_c.reshape(-1, F_), ACT_SILU)
    R.check(y.reshape(-1, F_), ref["y"], ref["y_cond"], BF16, "3d y")
    R.check(dx.reshape(-1, 2 * F_)[:, :F_], ref["dgate"], ref["dgate_cond"], BF16, "3d dgate")
    R.check(dx.reshape(-1, 2 * F_)[:, F_:], ref["dup"], ref["dup_cond"], BF16, "3d dup")
    R.check_dbias(db, ref, F32, B * S, "3d dbias")
    # non-contiguous input: the same bits as its contiguous copy, and the view is left alone
    wide = torch.cat([x, x], -1)
    view = wide[..., :2 * F_]
    assert not view.is_contiguous()
    y2, dx2, _ = _autograd(view, b, dy, ACT_SILU)
    assert torch.equal(y2, y) and torch.equal(dx2, dx) and torch.equal(wide[..., 2 * F_:], x)
    # a bias without requires_grad: no bias gradient is computed
    xr = x.clone().requires_grad_(True)
    fops.bias_swiglu(xr, b).backward(dy)
    assert torch.equal(xr.grad, dx) and b.grad is None
    # GEGLU wrappers reach their activation codes
    assert torch.equal(fops.bias_geglu(x, b), fops.gated_act(x, b, ACT_GELU))
    assert torch.equal(fops.bias_geglu(x, b, approximate="tanh"), fops.gated_act(x, b, ACT_GELU_TANH))


@pytest.mark.parametrize("xdt,bdt", [(F32, F32), (BF16, F32), (F16, F16)])
def test_bias_act_silu(xdt, bdt):
    """ACT_SILU through the plain bias_act kernels: y = silu(x + b), dx = dy silu'(x + b)."""
    C = _C()
    g = torch.Generator().manual_seed(8)
    rows, cols = 17, 2056
    x_c = (torch.randn((rows, cols), generator=g) * 4).to(xdt)
    b_c = torch.randn((cols,), generator=g).to(bdt)
    dy_c = torch.randn((rows, cols), generator=g).to(xdt)
    y = C.bias_act_fwd(x_c.to(DEV), b_c.to(DEV), ACT_SILU)
    dx, db = C.bias_act_bwd(dy_c.to(DEV), x_c.to(DEV), b_c.to(DEV), ACT_SILU)
    ca = x_c.double().abs() + b_c.double().abs()
    f, fp, cf, cfp = R.ref_act(x_c.double() + b_c.double(), ACT_SILU)
    d = dy_c.double()
    R.check(y, f, cf + fp.abs() * ca, xdt, "bias_act silu y", f"bias_act silu/y/{R.DT_NAME[xdt]}")
    R.check(dx, d * fp, d.abs() * cfp, xdt, "bias_act silu dx", f"bias_act silu/dx/{R.DT_NAME[xdt]}")
    ref = {"dbias": (d * fp).sum(0), "dbias_cond": (d.abs() * cfp).sum(0)}
    R.check_dbias(db, ref, bdt, rows, "bias_act silu dbias", f"bias_act silu/dbias/{R.DT_NAME[bdt]}")
