"""The sigmoid router's kernels (csrc/moe_route.hip) through apex.ops.moe_route and MoEMLP, against float64.

Inputs, reference and the derivation of every bound: tests/moe_sigmoid_reference.py. Ids, counts and row maps are
compared exactly.

Layer test: per tensor max |got - ref| / max |ref| against the dense float64 formulation, allowed twice what the
same layer with the PyTorch routing (moe_route(fused=False), same GEMMs, inputs and seed) measured against that
reference on an MI355X: out 6.18e-3, dx 5.54e-3, drouter 4.16e-3, dw1 3.96e-3, dw2 6.56e-3.
"""
import pytest
import torch
import torch.nn.functional as F

from mt_reference import BF16, DT_NAME, F32, HALF_ULP, TINY
from gemm_reference import E24, check
from moe_sigmoid_reference import CASES, SCALE, backward_bounds, case, forward_bounds, route64

pytestmark = pytest.mark.gpu

params = pytest.mark.parametrize("dt,T,E,topk,G,gtopk,with_bias",
                                 [(dt,) + c + (True,) for dt in (F32, BF16) for c in CASES] + [(BF16,) + CASES[1] + (False,)],
                                 ids=lambda v: DT_NAME.get(v, str(v)))
TORCH_ROUTING_ERR = {"out": 6.18e-3, "dx": 5.54e-3, "drouter": 4.16e-3, "dw1": 3.96e-3, "dw2": 6.56e-3}


def reference(T, E, topk, G, gtopk, with_bias):
    lg, bias, l64, ref = case(T, E, topk, G, gtopk)
    return (lg, bias, l64, ref) if with_bias else (lg, None, l64, route64(l64, None, topk, G, gtopk))


def route(lg, bias, topk, G, gtopk, aux):
    from apex.ops import moe_route

    return moe_route(lg, topk, aux_loss=aux, fused=True, score_function="sigmoid", scaling_factor=SCALE,
                     expert_bias=None if bias is None else bias.cuda(), num_groups=G or None, group_topk=gtopk or None)


@params
def test_forward(dt, T, E, topk, G, gtopk, with_bias):
    from apex.ops.grouped import _routing_maps

    lg, bias, l64, (ids, probs, _, _, counts, aux) = reference(T, E, topk, G, gtopk, with_bias)
    r = route(lg.to(dt).cuda(), bias, topk, G, gtopk, True)
    assert r.expert_ids.dtype == r.tokens_per_expert.dtype == torch.int32 and r.probs.dtype == torch.float32
    assert torch.equal(r.expert_ids.cpu().long(), ids) and torch.equal(r.tokens_per_expert.cpu().long(), counts)
    offsets, dest, token_of_row, R = _routing_maps(ids, E)
    assert torch.equal(r.offsets.cpu(), offsets) and torch.equal(r.dest.cpu(), dest)
    assert torch.equal(r.token_of_row.cpu(), token_of_row)
    want = torch.zeros(R).scatter_(0, dest.reshape(-1).long(), r.probs.detach().cpu().reshape(-1))
    assert torch.equal(r.row_prob.cpu(), want)             # probs at dest, bitwise; zero elsewhere
    b_p, b_a = forward_bounds(l64, ids, probs, aux, topk)
    what = f"{DT_NAME[dt]} T{T} E{E} topk{topk} G{G}"
    check(r.probs, probs.detach(), b_p + TINY[F32], what + " probs")
    check(r.aux_loss.reshape(1), aux.detach().reshape(1), b_a, what + " aux")


@params
def test_backward(dt, T, E, topk, G, gtopk, with_bias):
    lg, bias, l64, (ids, probs, s, n, counts, aux) = reference(T, E, topk, G, gtopk, with_bias)
    gp, ga = torch.randn(T, topk, generator=torch.Generator().manual_seed(7)), 0.75
    b_gate, b_aux = backward_bounds(l64, ids, probs, s, n, counts, gp.double(), ga, topk)
    chosen = torch.zeros(T, E, dtype=torch.bool).scatter_(1, ids, True)
    for use_aux in (True, False):
        ld = lg.to(dt).cuda().requires_grad_()
        r = route(ld, bias, topk, G, gtopk, use_aux)
        (dl,) = torch.autograd.grad((r.probs * gp.cuda()).sum() + (ga * r.aux_loss if use_aux else 0.0), ld)
        (ref,) = torch.autograd.grad((probs * gp.double()).sum() + (ga * aux if use_aux else 0.0), l64,
                                     retain_graph=True)
        bound = b_gate + (b_aux if use_aux else 0.0) + (E24 + (HALF_ULP[dt] if dt != F32 else 0.0)) * ref.abs() + TINY[dt]
        assert dl.dtype == dt
        check(dl, ref, bound, f"{DT_NAME[dt]} T{T} E{E} topk{topk} G{G} aux{use_aux} dlogits")
        if not use_aux:
            assert not dl.cpu()[~chosen].any()             # experts a token did not choose: exactly zero


def layer_case():
    """The layer test's module and inputs (also what the PyTorch routing's error was measured on)."""
    from apex.transformer.moe import MoEMLP

    torch.manual_seed(5)
    m = MoEMLP(64, 128, 8, 2, "swiglu", init_std=0.3, params_dtype=BF16, score_function="sigmoid", num_groups=4,
               group_topk=2, expert_bias=True).cuda()
    m.expert_bias.copy_(torch.tensor([1, -2, 0, 3, -1, 2, 0, -3]) / 8)
    x = torch.randn(300, 64).to(BF16).cuda().requires_grad_()
    return m, x, torch.randn(300, 64).to(BF16).cuda()


def layer_errors(m, x, dout, out, ids):
    """{tensor: max |got - ref| / max |ref|} of out and the gradients of x, router.weight, w1, w2."""
    params = [x, m.router.weight, m.w1, m.w2]
    got = (out,) + torch.autograd.grad(out, params, dout)
    x64, wr, w1, w2 = p64 = [t.detach().double().cpu().requires_grad_() for t in params]
    probs = route64(x64 @ wr.t(), None, 2, 4, 2, ids, scale=1.0)[1]
    ref = torch.zeros_like(x64)
    for e in range(8):
        gate, up = (x64 @ w1[e].t()).chunk(2, -1)
        ref = ref + (probs * (ids == e)).sum(-1, keepdim=True) * ((F.silu(gate) * up) @ w2[e].t())
    refs = (ref,) + torch.autograd.grad((ref * dout.double().cpu()).sum(), p64)
    return {n: float((g.detach().double().cpu() - r.detach()).abs().max() / r.detach().abs().max())
            for n, g, r in zip(TORCH_ROUTING_ERR, got, refs)}


def test_layer():
    m, x, dout = layer_case()
    out, _ = m(x)
    lg = m.router(x).float().detach().cpu().double()
    ids, probs, _, _, counts, _ = route64(lg, m.expert_bias.cpu(), 2, 4, 2, scale=1.0)
    assert torch.equal(m.expert_ids.cpu(), ids) and torch.equal(m.tokens_per_expert.cpu(), counts)
    assert torch.equal(m.tokens_per_expert_acc.cpu(), counts.float())
    check(m.router_probs, probs, forward_bounds(lg, ids, probs, probs.sum(), 2)[0] + TINY[F32], "router_probs")
    errs = layer_errors(m, x, dout, out, ids)
    print(errs)
    for name, err in errs.items():
        assert err <= 2 * TORCH_ROUTING_ERR[name], (name, err, TORCH_ROUTING_ERR[name])
