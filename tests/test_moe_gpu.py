"""The MoE row kernels (csrc/moe.hip) through apex.ops.moe_permute / moe_unpermute, forward and both backwards,
against float64.

T = 96 tokens, E = 5 experts, expert 3 never chosen (an empty segment), the other counts not multiples of 64
(pad rows in every segment). H = 64: one 16-byte chunk per lane in use on 8 lanes; H = 200: 25 chunks, a
partial wave.

Bounds, from the kernels' operation order (u = HALF_ULP[T]):
  combine  acc = fma(w_k, src_k, acc) over k in fp32, rounded once to T: at most one fp32 rounding per product and
           topk fp32 additions of partial sums that sum_k |w src| bounds, so
           (topk + 1) 2^-24 sum_k |w src| + u |ref| + TINY[T] (the fused multiply-add only removes roundings).
  gather   with scale: one fp32 product, rounded to T: the same expression with one term.
  dw       <g, src> over H exact products of 16-bit values, H fp32 additions in any order (lane partials, then
           the wave butterfly): H 2^-24 sum |g src|.
"""
import pytest
import torch

from mt_reference import BF16, DT_NAME, F16, HALF_ULP, TINY
from gemm_reference import E24, check

pytestmark = pytest.mark.gpu

T, E = 96, 5
params = pytest.mark.parametrize("dt,H,topk", [(dt, H, k) for dt in (BF16, F16) for H in (64, 200) for k in (1, 2)],
                                 ids=lambda v: DT_NAME.get(v, str(v)))


def routing(topk):
    g = torch.Generator().manual_seed(11 + topk)
    scores = torch.rand(T, E, generator=g)
    scores[:, 3] = -1.0                                    # expert 3 gets no token
    ids = scores.topk(topk, -1).indices
    counts = torch.bincount(ids.reshape(-1), minlength=E)
    assert counts[3] == 0 and (counts % 64 != 0).any()
    ends = torch.cumsum((counts + 63) // 64 * 64, 0)
    return ids, counts, torch.cat([ends.new_zeros(1), ends])


def bound(terms_abs, nterms, ref, dt):
    return (nterms + 1) * E24 * terms_abs + HALF_ULP[dt] * ref.abs() + TINY[dt]


@params
def test_permute(dt, H, topk):
    from apex.ops import moe_permute

    ids, counts, offsets = routing(topk)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(1)).to(dt)
    xp, off, dest = moe_permute(x.cuda(), ids.cuda(), E)
    R = (T * topk + 63) // 64 * 64 + 64 * E
    assert xp.shape == (R, H) and off.dtype == dest.dtype == torch.int32
    assert torch.equal(off.cpu().long(), offsets)
    xp, dest = xp.cpu(), dest.cpu().long()
    first = offsets[ids]                                   # every copy inside its expert's segment, no row twice
    assert ((dest >= first) & (dest < first + counts[ids])).all() and dest.unique().numel() == T * topk
    assert torch.equal(xp[dest], x[:, None, :].expand(T, topk, H))   # mapped rows: bit-equal
    mapped = torch.zeros(R, dtype=torch.bool)
    mapped[dest.reshape(-1)] = True
    assert not xp[~mapped].any()                           # pad and tail rows: exactly zero


@params
def test_unpermute_and_backwards(dt, H, topk):
    from apex.ops import moe_permute, moe_unpermute

    ids, _, _ = routing(topk)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(T, H, generator=g).to(dt)
    xd = x.cuda().requires_grad_()
    xp, _, dest = moe_permute(xd, ids.cuda(), E)
    R, d = xp.shape[0], dest.cpu().long()
    yp, dxp = torch.randn(R, H, generator=g).to(dt), torch.randn(R, H, generator=g).to(dt)
    probs = torch.softmax(torch.randn(T, topk, generator=g), -1)
    dout = torch.randn(T, H, generator=g).to(dt)
    ypd, pd = yp.cuda().requires_grad_(), probs.cuda().requires_grad_()
    out = moe_unpermute(ypd, dest, pd)
    dyp, dprobs = torch.autograd.grad(out, [ypd, pd], dout.cuda())
    (dx,) = torch.autograd.grad(xp, xd, dxp.cuda())
    what = f"{DT_NAME[dt]} H{H} topk{topk}"

    terms = probs.double()[..., None] * yp.double()[d]     # [T, topk, H]
    check(out, terms.sum(1), bound(terms.abs().sum(1), topk, terms.sum(1), dt), what + " unpermute")
    # permute backward: the plain sum of the top-k rows of the upstream gradient
    rows = dxp.double()[d]
    check(dx, rows.sum(1), bound(rows.abs().sum(1), topk, rows.sum(1), dt), what + " permute backward")
    # unpermute backward: dyp[dest[t, k]] = probs[t, k] * dout[t]; unmapped rows exactly zero
    ref = torch.zeros(R, H, dtype=torch.float64)
    ref[d.reshape(-1)] = (probs.double()[..., None] * dout.double()[:, None, :]).reshape(-1, H)
    check(dyp, ref, bound(ref.abs(), 1, ref, dt), what + " unpermute backward")
    mapped = torch.zeros(R, dtype=torch.bool)
    mapped[d.reshape(-1)] = True
    assert not dyp.cpu()[~mapped].any()
    prod = dout.double()[:, None, :] * yp.double()[d]
    assert dprobs.dtype == torch.float32
    check(dprobs, prod.sum(-1), H * E24 * prod.abs().sum(-1), what + " dprobs")
