"""CPU tier of the gated-activation tests: the PyTorch formulation (apex.ops.fused.gated_act_reference, the
path CPU tensors take) against the float64 reference of glu_reference.py by its bound, float64
gradcheck, and mutants of the formulas that the bound must reject."""
import pytest
import torch

import glu_reference as R
from apex.ops import fused as fops
from glu_reference import ACT_GELU, ACT_GELU_TANH, ACT_SILU, ACTS, F32, GLU_CASES


def _run(fn, case, x=None, bias=None, dy=None):
    """(y, dx, dbias or None) of fn(x, bias, act) and its autograd gradients on the case's inputs."""
    x0, b0, dy0 = R.glu_inputs(case)
    x = (x0 if x is None else x).clone().requires_grad_(True)
    bias = b0 if bias is None else bias
    b = bias.clone().requires_grad_(True) if bias is not None else None
    y = fn(x, b, case.act)
    y.backward(dy0 if dy is None else dy)
    return y.detach(), x.grad, (b.grad if b is not None else None)


@pytest.mark.parametrize("name", list(GLU_CASES))
def test_reference_path_inside_bound(name):
    case = GLU_CASES[name]
    y, dx, db = _run(fops.gated_act_reference, case)
    assert y.dtype == case.xdt and dx.dtype == case.xdt and (db is None or db.dtype == case.bdt)
    R.check_all(case, y, dx, db)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("with_bias", [False, True])
def test_gradcheck_float64(act, with_bias):
    g = torch.Generator().manual_seed(11 + act)
    x = (torch.randn((3, 16), generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    b = torch.randn((16,), generator=g, dtype=torch.float64).requires_grad_(True) if with_bias else None
    inputs = (x, b) if with_bias else (x,)
    fn = (lambda x_, b_: fops.gated_act(x_, b_, act)) if with_bias else (lambda x_: fops.gated_act(x_, None, act))
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-8, rtol=1e-6)


def test_gated_act_on_cpu_is_the_reference_path():
    for name in ("glu/silu-f32-bf32-r17-F8-randn4", "glu/geluerf-bf16-bbf16-r17-F8-pm80"):
        case = GLU_CASES[name]
        got = _run(fops.gated_act, case)
        want = _run(fops.gated_act_reference, case)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    x, b, _ = R.glu_inputs(GLU_CASES["glu/silu-f32-bf32-r17-F8-randn4"])
    assert torch.equal(fops.bias_swiglu(x, b), fops.gated_act_reference(x, b, ACT_SILU))
    assert torch.equal(fops.bias_geglu(x, b), fops.gated_act_reference(x, b, ACT_GELU))
    assert torch.equal(fops.bias_geglu(x, b, approximate="tanh"), fops.gated_act_reference(x, b, ACT_GELU_TANH))
    assert torch.equal(fops.gated_act(x), fops.gated_act_reference(x, None, ACT_SILU))
    from apex.transformer.functional import bias_swiglu

    assert bias_swiglu is fops.bias_swiglu
    assert torch.equal(fops._act_ref(x, ACT_SILU), torch.nn.functional.silu(x))
    with pytest.raises(ValueError):
        fops.gated_act(x, b, fops.ACT_RELU)
    with pytest.raises(ValueError):
        fops.bias_geglu(x, b, approximate="erf")
    with pytest.raises(ValueError):
        fops.gated_act(x[:, :15])


# ----------------------------------------------------------------------------
# mutants: each is a wrong formula (or a wrong number of roundings) that check must reject
# ----------------------------------------------------------------------------
def _act32(a, act):
    return fops._act_ref(a, act)


def _mut_halves_swapped(x, b, act):
    h = x.float() + (b.float() if b is not None else 0.0)
    up, gate = h.chunk(2, -1)
    return (_act32(gate, act) * up).to(x.dtype)


def _mut_bias_wrong_half(x, b, act):
    F_ = x.shape[-1] // 2
    h = x.float() + torch.cat([b.float()[F_:], b.float()[:F_]])
    gate, up = h.chunk(2, -1)
    return (_act32(gate, act) * up).to(x.dtype)


def _mut_rounded_twice(x, b, act):
    h = x.float() + b.float()
    gate, up = h.chunk(2, -1)
    return (_act32(gate, act).to(x.dtype).float() * up).to(x.dtype)


class _SiluGradMutant(torch.autograd.Function):
    """SwiGLU with a hand-written backward; kind "noterm": act' = sigma (the a (1 - sigma) term missing);
    kind "dup": dup = dy act'(a) instead of dy act(a)."""

    @staticmethod
    def forward(ctx, x, b, kind):
        ctx.save_for_backward(x, b)
        ctx.kind = kind
        a, v = (x + b).chunk(2, -1)
        return torch.nn.functional.silu(a) * v

    @staticmethod
    def backward(ctx, dy):
        x, b = ctx.saved_tensors
        a, v = (x + b).chunk(2, -1)
        s = torch.sigmoid(a)
        fp = s if ctx.kind == "noterm" else s * (1 + a * (1 - s))
        dup = dy * (fp if ctx.kind == "dup" else a * s)
        dx = torch.cat([dy * v * fp, dup], -1)
        return dx, dx.sum(0), None


def _rejected(case, y=None, dx=None, db=None):
    good = _run(fops.gated_act_reference, case)
    y, dx, db = (good[0] if y is None else y), (good[1] if dx is None else dx), (good[2] if db is None else db)
    with pytest.raises(AssertionError):
        R.check_all(case, y, dx, db)


def test_check_rejects_mutants():
    case = GLU_CASES["glu/silu-f32-bf32-r17-F8-randn4"]
    assert case.xdt == F32 and case.act == ACT_SILU
    R.check_all(case, *_run(fops.gated_act_reference, case))
    _rejected(case, y=_run(_mut_halves_swapped, case)[0])
    _rejected(case, y=_run(_mut_bias_wrong_half, case)[0])
    for kind in ("noterm", "dup"):
        y, dx, db = _run(lambda x, b, act, kind=kind: _SiluGradMutant.apply(x, b, kind), case)
        ref = R.glu_reference(case.name)
        R.check(y, ref["y"], ref["y_cond"], case.xdt)   # the forward is right, so only the gradient is caught
        _rejected(case, dx=dx)
        _rejected(case, db=db)
    # one rounding too many, in a 16-bit case (in fp32 a second fp32 rounding is no mutant)
    c16 = GLU_CASES["glu/silu-bf16-bbf16-r17-F8-randn4"]
    R.check_all(c16, *_run(fops.gated_act_reference, c16))
    _rejected(c16, y=_run(_mut_rounded_twice, c16)[0])
    # a non-finite value anywhere
    y = _run(fops.gated_act_reference, case)[0].clone()
    for bad in (float("nan"), float("inf")):
        y[3, 5] = bad
        _rejected(case, y=y)
    db = _run(fops.gated_act_reference, case)[2].clone()
    db[2] = float("nan")
    _rejected(case, db=db)
