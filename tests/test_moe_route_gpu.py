"""The routing kernels (csrc/moe_route.hip) through apex.ops.moe_route and MoEMLP, against float64.

Logits are randn rounded to multiples of 1/4 (frequent ties, exact in bf16). Ids, counts and row maps are exact:
the stable descending sort and ``_routing_maps`` on the CPU. Bounds of the float outputs, from the kernels'
operation order (all fp32; e = 2^-24; d = the spread of the logits that enter the softmax, per row):
  probs  exp(v_k - m): the subtraction rounds (|d| e relative on the exponential), expf is within 1 ulp (2 e);
         topk additions of positive terms (topk e); one correctly rounded division (e):
         eps_p = (2 d + topk + 5) e relative, numerator and denominator counted separately.
  aux    the full softmax likewise with E additions: eps_s = (2 d + E + 5) e; its per-expert sum over T tokens in
         a fixed order (T e); counts are exact; E products and additions and the scale (E + 3) e; all terms are
         positive, so (eps_s + (T + E + 3) e) relative.
  dlogits  p_k (dp_k - sum_m p_m dp_m): the stored p carry eps_p, the dot product topk + 1 roundings, the
         subtraction and the product one each: (2 eps_p + (topk + 4) e) p_k (|dp_k| + sum_m p_m |dp_m|);
         d_aux scale s_j (c_j - sum_e s_e c_e): (2 eps_s + (E + 6) e) |d_aux| scale s_j (c_j + sum_e s_e c_e);
         the sum of the two parts (e |ref|) and the rounding to the logits' dtype (half an ulp).

Layer test: per tensor max |got - ref| / max |ref| against the dense float64 formulation, allowed twice what the
parent commit's layer (torch routing, aux_loss_coeff = 0, same inputs and seed) measured against that reference
on an MI355X: out 6.20e-3, dx 8.70e-3, drouter 4.49e-3, dw1 5.99e-3, dw2 4.50e-3.
"""
import pytest
import torch
import torch.nn.functional as F

from mt_reference import BF16, DT_NAME, F32, HALF_ULP, TINY
from gemm_reference import E24, check

pytestmark = pytest.mark.gpu

CASES = [(300, 5, 2), (257, 64, 8), (64, 256, 1), (1, 8, 2), (1000, 200, 4)]
params = pytest.mark.parametrize("dt,T,E,topk", [(dt,) + c for dt in (F32, BF16) for c in CASES],
                                 ids=lambda v: DT_NAME.get(v, str(v)))
PARENT_ERR = {"out": 6.20e-3, "dx": 8.70e-3, "drouter": 4.49e-3, "dw1": 5.99e-3, "dw2": 4.50e-3}


def make_logits(T, E, dt):
    lg = (torch.randn(T, E, generator=torch.Generator().manual_seed(1000 * T + E)) * 4).round() / 4
    if E == 5:
        lg[:, 3] = -30.0                                   # expert 3 gets no token: an empty segment
    return lg.to(dt)


def route64(l64, topk, ids=None):
    """(ids, probs, full softmax, counts, aux) in float64; ids from the stable sort unless given."""
    T, E = l64.shape
    if ids is None:
        ids = torch.sort(l64, dim=-1, descending=True, stable=True).indices[:, :topk]
    probs, s = torch.softmax(l64.gather(1, ids), -1), torch.softmax(l64, -1)
    counts = torch.bincount(ids.reshape(-1), minlength=E)
    return ids, probs, s, counts, E / (T * T * topk) * (counts.double() * s.sum(0)).sum()


def eps(l64, ids, topk):
    """(eps_p [T, 1], eps_s [T, 1]) of the module docstring."""
    top = l64.gather(1, ids)
    d_p = top[:, :1] - top[:, -1:]
    d_s = l64.max(-1, keepdim=True).values - l64.min(-1, keepdim=True).values
    return (2 * d_p + topk + 5) * E24, (2 * d_s + l64.shape[1] + 5) * E24


@params
def test_forward(dt, T, E, topk):
    from apex.ops import moe_route
    from apex.ops.grouped import _routing_maps

    lg = make_logits(T, E, dt)
    r = moe_route(lg.cuda(), topk, aux_loss=True, fused=True)
    ids, probs, _, counts, aux = route64(lg.double(), topk)
    assert r.expert_ids.dtype == r.tokens_per_expert.dtype == torch.int32 and r.probs.dtype == torch.float32
    assert torch.equal(r.expert_ids.cpu().long(), ids) and torch.equal(r.tokens_per_expert.cpu().long(), counts)
    if E == 5:
        assert counts[3] == 0
    offsets, dest, token_of_row, R = _routing_maps(ids, E)
    assert torch.equal(r.offsets.cpu(), offsets) and torch.equal(r.dest.cpu(), dest)
    assert torch.equal(r.token_of_row.cpu(), token_of_row)
    want = torch.zeros(R).scatter_(0, dest.reshape(-1).long(), r.probs.detach().cpu().reshape(-1))
    assert torch.equal(r.row_prob.cpu(), want)             # probs at dest, bitwise; zero elsewhere
    eps_p, eps_s = eps(lg.double(), ids, topk)
    what = f"{DT_NAME[dt]} T{T} E{E} topk{topk}"
    check(r.probs, probs, eps_p * probs + TINY[F32], what + " probs")
    check(r.aux_loss.reshape(1), aux.reshape(1), (eps_s.max() + (T + E + 3) * E24) * aux.reshape(1), what + " aux")


@params
def test_backward(dt, T, E, topk):
    from apex.ops import moe_route

    lg = make_logits(T, E, dt)
    g = torch.Generator().manual_seed(7)
    gp, ga = torch.randn(T, topk, generator=g), 0.75
    l64 = lg.double().requires_grad_()
    ids, probs, s, counts, aux = route64(l64, topk)
    eps_p, eps_s = eps(l64.detach(), ids, topk)
    p, s, c = probs.detach(), s.detach(), counts.double()
    b_gate = torch.zeros(T, E, dtype=torch.float64).scatter_(
        1, ids, (2 * eps_p + (topk + 4) * E24) * p * (gp.abs() + (p * gp.abs()).sum(-1, keepdim=True)))
    b_aux = (2 * eps_s + (E + 6) * E24) * ga * E / (T * T * topk) * s * (c + (s * c).sum(-1, keepdim=True))
    chosen = torch.zeros(T, E, dtype=torch.bool).scatter_(1, ids, True)
    for use_aux in (True, False):
        ld = lg.cuda().requires_grad_()
        r = moe_route(ld, topk, aux_loss=use_aux, fused=True)
        loss = (r.probs * gp.cuda()).sum() + (ga * r.aux_loss if use_aux else 0.0)
        (dl,) = torch.autograd.grad(loss, ld)
        (ref,) = torch.autograd.grad((probs * gp.double()).sum() + (ga * aux if use_aux else 0.0), l64,
                                     retain_graph=True)
        bound = b_gate + (b_aux if use_aux else 0.0) + (E24 + (HALF_ULP[dt] if dt != F32 else 0.0)) * ref.abs() + TINY[dt]
        assert dl.dtype == dt
        check(dl, ref, bound, f"{DT_NAME[dt]} T{T} E{E} topk{topk} aux{use_aux} dlogits")
        if not use_aux:
            assert not dl.cpu()[~chosen].any()             # experts a token did not choose: exactly zero


def layer_case():
    """The layer test's module and inputs (also what the parent commit's error was measured on)."""
    from apex.transformer.moe import MoEMLP

    torch.manual_seed(5)
    m = MoEMLP(64, 128, 5, 2, "swiglu", init_std=0.3, params_dtype=BF16, aux_loss_coeff=0.01).cuda()
    x = torch.randn(300, 64).to(BF16).cuda().requires_grad_()
    return m, x, torch.randn(300, 64).to(BF16).cuda()


def dense64(x, wr, w1, w2, ids, coeff):
    """tests/test_moe.py's dense formulation (swiglu) with given ids; returns (out, coeff * aux)."""
    logits = x @ wr.t()
    _, probs, _, _, aux = route64(logits, ids.shape[1], ids)
    out = torch.zeros_like(x)
    for e in range(w1.shape[0]):
        gate, up = (x @ w1[e].t()).chunk(2, -1)
        out = out + (probs * (ids == e)).sum(-1, keepdim=True) * ((F.silu(gate) * up) @ w2[e].t())
    return out, coeff * aux


def layer_errors(m, x, dout, out, ids, coeff):
    """{tensor: max |got - ref| / max |ref|} of out and the gradients of x, router.weight, w1, w2."""
    params = [x, m.router.weight, m.w1, m.w2]
    got = (out,) + torch.autograd.grad(out, params, dout)
    p64 = [t.detach().double().cpu().requires_grad_() for t in params]
    ref, aux = dense64(*p64, ids.cpu(), coeff)
    refs = (ref,) + torch.autograd.grad((ref * dout.double().cpu()).sum() + aux, p64)
    return {n: float((g.detach().double().cpu() - r.detach()).abs().max() / r.detach().abs().max())
            for n, g, r in zip(PARENT_ERR, got, refs)}, aux


def test_layer():
    m, x, dout = layer_case()
    out, _ = m(x)
    lg = m.router(x).float().detach().cpu().double()
    ids, probs, _, counts, aux = route64(lg, 2)
    assert m.expert_ids.dtype == m.tokens_per_expert.dtype == torch.int64
    assert torch.equal(m.expert_ids.cpu(), ids) and torch.equal(m.tokens_per_expert.cpu(), counts)
    eps_p, eps_s = eps(lg, ids, 2)
    check(m.router_probs, probs, eps_p * probs + TINY[F32], "router_probs")
    aux = 0.01 * aux.reshape(1)
    check(m.aux_loss.reshape(1), aux, (eps_s.max() + (300 + 5 + 4) * E24) * aux, "aux_loss")
    errs, _ = layer_errors(m, x, dout, out, ids, 0.01)
    print(errs)
    for name, err in errs.items():
        assert err <= 2 * PARENT_ERR[name], (name, err, PARENT_ERR[name])
