"""The sigmoid router's PyTorch formulation (apex/ops/grouped.py) against the float64 reference of
tests/moe_sigmoid_reference.py (fp32 torch ops: the bounds derived there for the kernels hold for them as well),
the argument checks, the untouched default path and MoEMLP's expert-bias update. No GPU."""
import pytest
import torch

from mt_reference import F32, TINY
from gemm_reference import check
from moe_sigmoid_reference import CASES, SCALE, case, forward_bounds


@pytest.mark.parametrize("T,E,topk,G,gtopk", [CASES[1], CASES[5]])
def test_torch_formulation(T, E, topk, G, gtopk):
    from apex.ops import moe_route
    from apex.ops.grouped import _routing_maps

    lg, bias, l64, (ids, probs, s, n, counts, aux) = case(T, E, topk, G, gtopk)
    ld = lg.clone().requires_grad_()
    r = moe_route(ld, topk, aux_loss=True, score_function="sigmoid", expert_bias=bias, num_groups=G, group_topk=gtopk,
                  scaling_factor=SCALE)
    assert torch.equal(r.expert_ids.long(), ids) and torch.equal(r.tokens_per_expert.long(), counts)
    for got, want in zip((r.offsets, r.dest, r.token_of_row), _routing_maps(ids, E)):
        assert torch.equal(got, want)
    b_p, b_a = forward_bounds(l64, ids, probs, aux, topk)
    check(r.probs, probs.detach(), b_p + TINY[F32], "probs")
    check(r.aux_loss.reshape(1), aux.detach().reshape(1), b_a, "aux")
    (dl,) = torch.autograd.grad(r.probs.sum(), ld)
    assert not dl[~torch.zeros(T, E, dtype=torch.bool).scatter_(1, ids, True)].any()


@pytest.mark.parametrize("kw", [dict(num_groups=4, group_topk=2), dict(score_function="sigmoid", num_groups=5, group_topk=2),
                                dict(score_function="sigmoid", num_groups=8, group_topk=1), dict(scaling_factor=2.0),
                                dict(expert_bias=torch.zeros(16))])
def test_value_errors(kw):
    from apex.ops import moe_route

    with pytest.raises(ValueError):                        # softmax with sigmoid options, E % G, topk > group_topk * E / G
        moe_route(torch.randn(4, 16), 4, **kw)


def test_defaults_unchanged():
    from apex.ops import moe_route
    from apex.ops.grouped import _route_reference

    lg = torch.randn(33, 12, generator=torch.Generator().manual_seed(1))
    for got, want in zip(moe_route(lg, 3, aux_loss=True), _route_reference(lg, 3, True)):
        assert torch.equal(got, want)


def test_update_expert_bias():
    from apex.transformer.moe import MoEMLP

    torch.manual_seed(0)
    m = MoEMLP(16, 32, 4, 2, score_function="sigmoid", expert_bias=True)
    m(torch.randn(50, 16))
    acc = m.tokens_per_expert_acc.clone()
    assert torch.equal(acc, m.tokens_per_expert.float()) and acc.sum() == 100
    m.update_expert_bias(0.5)
    assert torch.equal(m.expert_bias, 0.5 * torch.sign(acc.mean() - acc)) and not m.tokens_per_expert_acc.any()
