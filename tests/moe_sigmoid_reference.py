"""Float64 reference of the sigmoid router (apex.ops.moe_route, score_function="sigmoid") and the inputs its tests share.

Inputs: logits are randn rounded to multiples of 1/4 and clamped to +-8 (exact in bf16), the bias multiples of 1/8
in [-1/2, 1/2], so equal (logit, bias) pairs tie exactly in fp32 and fp64, and distinct keys on that grid are at
least 6.8e-5 apart (fp32 key error < 1e-6): the experts chosen are exact. With groups, group 1 carries group 0's
biases and every 97th row group 0's logits: exact group ties. ``case`` asserts that the two group scores at the cut
come from identical key pairs or differ by more than 2^-16 in every row; SEEDS are chosen so that this holds.

Bounds, from the kernels' operation order (all fp32, e = 2^-24):
  s      1 / (1 + expf(-x)): expf within 1 ulp (2 e, damped by u / (1 + u)), one addition, one division: eps_s = 5 e.
  probs  scale * s_k (eps_s + e) over the sum of topk positive terms plus 1e-20 (eps_s + (topk + 1) e), one
         division (e): eps_p = 2 eps_s + (topk + 3) e; topk == 1 has no denominator and stays below that.
  aux    s / (sum_e s + 1e-20): eps_n = 2 eps_s + (E + 2) e; then as the softmax router: T additions per expert,
         E products and additions and the scale: (eps_n + (T + E + 3) e) relative, every term positive.
  dlogits  (scale dp_k - sum_m p_m dp_m) / D * s_k (1 - s_k): the stored p carry eps_p, the dot product topk + 1
         roundings, scale dp and the subtraction one each, D eps_s + (topk + 1) e, the division e, s_k eps_s,
         1 - s_k eps_s s_k / (1 - s_k) + e, two products 2 e:
         (eps_p + 2 eps_s + (2 topk + 9) e + eps_s s_k / (1 - s_k)) on (scale |dp_k| + sum_m p_m |dp_m|) / D s_k (1 - s_k);
         the aux part d_aux scale_aux (c_j - sum_e n_e c_e) / N s_j (1 - s_j) likewise:
         (eps_n + 2 eps_s + (2 E + 11) e + eps_s s_j / (1 - s_j)) on its magnitude with c_j + sum_e n_e c_e;
         the sum of the two parts (e |ref|) and the rounding to the logits' dtype (half an ulp).
"""
import functools

import torch

from gemm_reference import E24

SCALE = 2.5
EPS_S = 5 * E24
# (T, E, topk, G, group_topk); G = 0: no groups. The last case is not a multiple of the 16-byte vector.
CASES = [(300, 8, 2, 0, 0), (257, 64, 8, 8, 4), (130, 256, 8, 8, 4), (64, 256, 1, 0, 0), (1, 16, 2, 4, 2),
         (259, 200, 4, 4, 2), (70, 13, 3, 0, 0)]
SEEDS = {(257, 64): 14, (130, 256): 4}                    # (T, E): seed; other cases take 1000 T + E


def route64(l64, bias, topk, G, gtopk, ids=None, scale=SCALE):
    """(ids, probs, s, normalised s, counts, aux) in float64; ids by the seven rules unless given."""
    T, E = l64.shape
    s = torch.sigmoid(l64)
    if ids is None:
        key = s.detach() + (0.0 if bias is None else bias.double())
        if G:
            top2 = key.view(T, G, E // G).topk(2, dim=-1).values
            gs, order = torch.sort(top2.sum(-1), dim=-1, descending=True, stable=True)
            if gtopk < G:                                  # the cut: identical key pairs, or clearly apart
                a, b = (top2.gather(1, order[:, k, None, None].expand(T, 1, 2)) for k in (gtopk - 1, gtopk))
                assert bool(((a == b).all(-1).squeeze(1) | (gs[:, gtopk - 1] - gs[:, gtopk] > 2.0 ** -16)).all())
            mask = torch.zeros(T, G, dtype=torch.bool).scatter_(1, order[:, :gtopk], True)
            key = key.masked_fill(~mask.repeat_interleave(E // G, dim=1), float("-inf"))
        ids = torch.sort(key, dim=-1, descending=True, stable=True).indices[:, :topk]
    sk = s.gather(1, ids)
    probs = scale * sk / (sk.sum(-1, keepdim=True) + 1e-20) if topk > 1 else scale * sk
    n = s / (s.sum(-1, keepdim=True) + 1e-20)
    counts = torch.bincount(ids.reshape(-1), minlength=E)
    return ids, probs, s, n, counts, E / (T * T * topk) * (counts.double() * n.sum(0)).sum()


@functools.lru_cache(maxsize=None)
def case(T, E, topk, G, gtopk):
    """(logits fp32, bias fp32, route64 of them with l64 requiring grad), built once per case."""
    g = torch.Generator().manual_seed(SEEDS.get((T, E), 1000 * T + E))
    lg = ((torch.randn(T, E, generator=g) * 4).round() / 4).clamp(-8, 8)
    bias = torch.randint(-4, 5, (E,), generator=g).float() / 8
    if G:
        S = E // G
        bias[S:2 * S] = bias[:S]
        lg[::97, S:2 * S] = lg[::97, :S]
    l64 = lg.double().requires_grad_()
    return lg, bias, l64, route64(l64, bias, topk, G, gtopk)


def forward_bounds(l64, ids, probs, aux, topk):
    """(bound of probs [T, topk], bound of aux [1])."""
    T, E = l64.shape
    eps_p, eps_n = 2 * EPS_S + (topk + 3) * E24, 2 * EPS_S + (E + 2) * E24
    return eps_p * probs.detach(), (eps_n + (T + E + 3) * E24) * aux.detach().reshape(1)


def backward_bounds(l64, ids, probs, s, n, counts, gp, ga, topk, scale=SCALE):
    """(gate part, aux part) of the dlogits bound [T, E] for dprobs = gp and d_aux = ga."""
    T, E = l64.shape
    s, n, p, c = s.detach(), n.detach(), probs.detach(), counts.double()
    sat = EPS_S * s / (1 - s)
    sk = s.gather(1, ids)
    D = sk.sum(-1, keepdim=True) + 1e-20 if topk > 1 else torch.ones(T, 1, dtype=torch.float64)
    mag = (scale * gp.abs() + ((p * gp.abs()).sum(-1, keepdim=True) if topk > 1 else 0.0)) / D * sk * (1 - sk)
    eps_p, eps_n = 2 * EPS_S + (topk + 3) * E24, 2 * EPS_S + (E + 2) * E24
    b_gate = torch.zeros(T, E, dtype=torch.float64).scatter_(
        1, ids, (eps_p + 2 * EPS_S + (2 * topk + 9) * E24 + sat.gather(1, ids)) * mag)
    N = s.sum(-1, keepdim=True) + 1e-20
    b_aux = (eps_n + 2 * EPS_S + (2 * E + 11) * E24 + sat) * ga * E / (T * T * topk) * \
        (c + (n * c).sum(-1, keepdim=True)) / N * s * (1 - s)
    return b_gate, b_aux
