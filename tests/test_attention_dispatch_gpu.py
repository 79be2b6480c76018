"""Every launch site of the 16-bit flash-attention dispatch (csrc/attention_impl.h), forward plus
backward, against the fp32 PyTorch reference of test_attention_gpu.py.

The product head dim x S x causal x dropout x bias x dtype reaches each forward variant and each
backward kernel combination the launchers can choose:

* S = 96 (one partial pair of 64-key tiles): the single-stage short forward at head dim 64 without a
  bias, the two-barrier forward elsewhere; the fused single-key-block backward;
* S = 160 (more than 128 keys, ragged last tile): the double-buffered forward at head dims 128 / 256
  and at 64 without dropout, the two-barrier forward elsewhere; the delta pre-pass + dK/dV + dQ
  backward with two key blocks.

With dropout the reference is the masked one, the mask taken from the mask debug kernel as in
test_flash_dropout_matches_masked_reference. The bias is ALiBi-style, [1, H, 1, S]: it depends on
head and key only, so the reference takes it as one more head-dim column (q' = [q, 1],
k' = [k, bias / scale]: q' . k' * scale = q . k * scale + bias) and stays the one of
test_attention_gpu.py.
"""
import math

import pytest
import torch

from test_attention_gpu import _ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H = 1, 2


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "alibi"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("S", [96, 160])
@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_dispatch_fwd_bwd(D, S, causal, p, with_bias, dt):
    import apex._ext as e
    from apex.contrib.multihead_attn import flash
    from apex.contrib.multihead_attn.attention import prepare_bias

    C = e.require()
    torch.manual_seed(1000 * D + S + int(causal))
    qkv = (torch.randn(B, S, 3, H, D, device=DEV) * 0.7).to(dt).requires_grad_(True)
    scale = 1.0 / math.sqrt(D)
    bias = None
    if with_bias:
        slopes = torch.tensor([2.0 ** -(h + 3) for h in range(H)], device=DEV)
        dist = torch.arange(S, device=DEV).float() - (S - 1)  # <= 0, 0 at the last key
        bias = prepare_bias((slopes[:, None] * dist[None, :])[None, :, None, :], B, H, S, S, dt)
        assert bias.shape == (1, H, 1, S)
    torch.manual_seed(11)
    o = flash.flash_attention_packed(qkv, p, causal, scale, None, bias)
    mask = None
    if p > 0:
        torch.manual_seed(11)
        seed, offset = flash._seed_pair(p, qkv.device)
        mask = C.flash_dropout_mask(B, H, S, S, p, seed, offset, qkv.device)
    do = torch.randn_like(o)
    o.backward(do)

    q, k, v = (t.float().clone() for t in qkv.detach().unbind(2))
    if with_bias:
        q = torch.cat([q, torch.ones(B, S, H, 1, device=DEV)], -1)
        k = torch.cat([k, (bias.float()[0, :, 0, :].t() / scale)[None, :, :, None]], -1)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    orf = _ref(q, k, v, causal, scale, mask=mask, p=round(p * 256) / 256)  # 8-bit dropout uniforms
    orf.backward(do.float())

    tol = 2e-2 if dt == torch.bfloat16 else 4e-3
    torch.testing.assert_close(o.float(), orf, rtol=tol, atol=tol)
    dq, dk, dv = qkv.grad.float().unbind(2)
    gtol = 5e-2 if dt == torch.bfloat16 else 1e-2
    torch.testing.assert_close(dv, v.grad, rtol=gtol, atol=gtol)
    torch.testing.assert_close(dk, k.grad[..., :D], rtol=gtol, atol=gtol)
    torch.testing.assert_close(dq, q.grad[..., :D], rtol=gtol, atol=gtol)
