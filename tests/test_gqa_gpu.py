"""Grouped-query attention on the GPU: the flash kernels with Hk < H key/value heads, the dK/dV group
reduction, the grouped packed Function, grouped RoPE and the GPT model option.

The exact tests rest on two facts. Forward, dQ and the per-query-head dK/dV of a grouped call are the
arithmetic of the MHA call on repeat_interleave'd K/V (only the K/V addresses differ), so they are
bit-equal. The reduction adds a group's heads in fp32 in ascending head order and rounds once, which
the tests redo with an explicit loop."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _C():
    import apex._ext as e

    return e.require()


def _rand(shape, dt, seed, s=0.8):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * s).to(dt).to(DEV)


def _fwd_bwd(q, k, v, do, causal, p, k_lens, bias, seed=5, offset=9):
    C = _C()
    scale = 1.0 / math.sqrt(q.shape[-1])
    o, lse, dmask = C.flash_attn_fwd(q, k, v, causal, scale, p, seed, offset, k_lens, bias)
    dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
    dbias = None if bias is None else torch.zeros(bias.shape, dtype=torch.float32, device=DEV)
    C.flash_attn_bwd(do, q, k, v, o, lse, dq, dk, dv, causal, scale, p, seed, offset, k_lens, dmask, None, 0, bias,
                     dbias=dbias)
    return o, lse, dq, dk, dv, dbias


def _group_sum(x, g):
    """[B, S, Hk * g, D] -> [B, S, Hk, D]: fp32, ascending head order, one rounding."""
    B, S, H, D = x.shape
    xg = x.view(B, S, H // g, g, D)
    acc = torch.zeros(B, S, H // g, D, dtype=torch.float32, device=x.device)
    for i in range(g):
        acc = acc + xg[:, :, :, i].float()
    return acc.to(x.dtype)


BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
EXACT = [
    # dt, B, Sq, Sk, H, Hk, D, causal, p, k_lens, bias
    pytest.param(BF, 2, 100, 100, 4, 2, 64, False, 0.0, None, False, id="bf16-one-key-block"),
    pytest.param(HF, 2, 100, 100, 4, 2, 64, False, 0.0, None, False, id="fp16-one-key-block"),
    pytest.param(BF, 1, 257, 257, 6, 2, 64, True, 0.0, None, False, id="bf16-two-kernel-g3"),
    pytest.param(BF, 1, 190, 190, 4, 1, 128, True, 0.0, None, False, id="bf16-mqa-d128"),
    pytest.param(BF, 2, 64, 160, 2, 1, 32, False, 0.0, [160, 77], False, id="bf16-klens-d32"),
    pytest.param(BF, 1, 136, 136, 2, 1, 256, False, 0.0, None, False, id="bf16-d256"),
    pytest.param(F32, 1, 130, 130, 4, 2, 64, False, 0.0, None, False, id="fp32"),
    pytest.param(BF, 2, 136, 136, 4, 2, 64, True, 0.1, None, False, id="bf16-dropout-causal"),
    pytest.param(BF, 1, 100, 100, 4, 2, 64, False, 0.0, None, True, id="bf16-trainable-bias"),
]


@pytest.mark.parametrize("dt,B,Sq,Sk,H,Hk,D,causal,p,k_lens,with_bias", EXACT)
def test_grouped_equals_expanded_mha(dt, B, Sq, Sk, H, Hk, D, causal, p, k_lens, with_bias):
    g = H // Hk
    q = _rand((B, Sq, H, D), dt, 1)
    k = _rand((B, Sk, Hk, D), dt, 2)
    v = _rand((B, Sk, Hk, D), dt, 3)
    do = _rand((B, Sq, H, D), dt, 4)
    kl = None if k_lens is None else torch.tensor(k_lens, dtype=torch.int32, device=DEV)
    bias = _rand((B, H, Sq, Sk), dt, 5, 0.5) if with_bias else None
    o, lse, dq, dk, dv, dbias = _fwd_bwd(q, k, v, do, causal, p, kl, bias)
    ke, ve = k.repeat_interleave(g, dim=2), v.repeat_interleave(g, dim=2)
    oe, lsee, dqe, dke, dve, dbiase = _fwd_bwd(q, ke, ve, do, causal, p, kl, bias)
    assert dk.shape == k.shape and dv.shape == v.shape
    assert torch.isfinite(o.float()).all() and float(dq.float().abs().max()) > 0
    assert torch.equal(o, oe)
    assert torch.equal(lse, lsee)
    assert torch.equal(dq, dqe)
    assert torch.equal(dk, _group_sum(dke, g))
    assert torch.equal(dv, _group_sum(dve, g))
    if with_bias:
        assert float(dbias.abs().max()) > 0 and torch.equal(dbias, dbiase)


@pytest.mark.parametrize("dt,B,S,Hk,g,D", [(BF, 2, 37, 3, 2, 64), (HF, 1, 50, 1, 8, 32), (F32, 3, 19, 2, 3, 128),
                                           (BF, 1, 300, 2, 5, 256)])
def test_kv_group_reduce_kernel(dt, B, S, Hk, g, D):
    """The reduction alone: strided outputs (the K and V slices of a packed gradient), several
    workgroups, a last workgroup that is not full; exact against the explicit fp32 loop."""
    C = _C()
    dk_x, dv_x = _rand((B, S, Hk * g, D), dt, 71, 1.0), _rand((B, S, Hk * g, D), dt, 72, 1.0)
    Hq = 5  # leading heads the reduction must leave alone
    packed = torch.full((B, S, Hq + 2 * Hk, D), 3.0, dtype=dt, device=DEV)
    dk, dv = packed[:, :, Hq:Hq + Hk], packed[:, :, Hq + Hk:]
    C.attn_kv_group_reduce(dk_x, dv_x, dk, dv)
    assert torch.equal(dk, _group_sum(dk_x, g))
    assert torch.equal(dv, _group_sum(dv_x, g))
    assert bool((packed[:, :, :Hq] == 3.0).all())


def _ref(q, k, v, causal, scale):
    """fp32 composition on [B, S, H, D] tensors (K/V already expanded to H heads)."""
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        cm = torch.ones(s.shape[-2], s.shape[-1], dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(cm, float("-inf"))
    pm = torch.nan_to_num(torch.softmax(s, -1))
    return torch.matmul(pm, vf).transpose(1, 2)


ACCURACY = [
    (BF, 2, 100, 4, 2, 64, False),
    (HF, 2, 100, 4, 2, 64, False),
    (BF, 1, 257, 6, 2, 64, True),
    (BF, 1, 190, 4, 1, 128, True),
]


@pytest.mark.parametrize("dt,B,S,H,Hk,D,causal", ACCURACY)
def test_attention_grouped_vs_fp32_composition(dt, B, S, H, Hk, D, causal):
    from apex.contrib.multihead_attn.attention import attention

    g = H // Hk
    q = _rand((B, S, H, D), dt, 11).requires_grad_(True)
    k = _rand((B, S, Hk, D), dt, 12).requires_grad_(True)
    v = _rand((B, S, Hk, D), dt, 13).requires_grad_(True)
    o = attention(q, k, v, causal=causal)
    do = _rand(o.shape, dt, 14, 1.0)
    o.backward(do)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    orf = _ref(qr, kr.repeat_interleave(g, dim=2), vr.repeat_interleave(g, dim=2), causal, 1.0 / math.sqrt(D))
    orf.backward(do.float())
    tol = 2e-2 if dt == BF else 4e-3
    gtol = 5e-2 if dt == BF else 1e-2
    assert k.grad.shape == k.shape and v.grad.shape == v.shape
    torch.testing.assert_close(o.float(), orf, rtol=tol, atol=tol)
    torch.testing.assert_close(v.grad.float(), vr.grad, rtol=gtol, atol=gtol)
    torch.testing.assert_close(k.grad.float(), kr.grad, rtol=gtol, atol=gtol)
    torch.testing.assert_close(q.grad.float(), qr.grad, rtol=gtol, atol=gtol)


@pytest.mark.parametrize("H,Hk,S,causal", [(4, 2, 100, False), (6, 2, 257, True), (4, 1, 190, True)])
def test_grouped_packed_function_matches_separate_views(H, Hk, S, causal):
    from apex.contrib.multihead_attn import flash

    B, D = 2, 64
    qkv = _rand((B, S, H + 2 * Hk, D), BF, 21).requires_grad_(True)
    o = flash.flash_attention_grouped_packed(qkv, H, Hk, 0.0, causal)
    do = _rand(o.shape, BF, 22, 1.0)
    o.backward(do)
    x = qkv.detach().clone().requires_grad_(True)
    o2 = flash.flash_attention(x[:, :, :H], x[:, :, H:H + Hk], x[:, :, H + Hk:], 0.0, causal)
    o2.backward(do)
    assert torch.equal(o, o2)
    assert qkv.grad.shape == qkv.shape and float(qkv.grad[:, :, H:].float().abs().max()) > 0
    assert torch.equal(qkv.grad, x.grad)


def test_grouped_packed_gradient_stays_inside_its_buffer():
    """dQ (kernel stores) and dK / dV (strided reduce stores) written into the slices of one packed
    gradient that sits inside a larger sentinel-filled buffer: the guards stay untouched."""
    C = _C()
    B, S, H, Hk, D = 2, 150, 4, 2, 64
    T = H + 2 * Hk
    qkv = _rand((B, S, T, D), BF, 31)
    q, k, v = qkv[:, :, :H], qkv[:, :, H:H + Hk], qkv[:, :, H + Hk:]
    do = _rand((B, S, H, D), BF, 32, 1.0)
    scale = 1.0 / math.sqrt(D)
    o, lse, dmask = C.flash_attn_fwd(q, k, v, True, scale, 0.0, 0, 0, None, None)
    n, pad, sentinel = qkv.numel(), 4096, 7.0
    buf = torch.full((pad + n + pad,), sentinel, dtype=BF, device=DEV)
    dqkv = buf[pad:pad + n].view(B, S, T, D)
    C.flash_attn_bwd(do, q, k, v, o, lse, dqkv[:, :, :H], dqkv[:, :, H:H + Hk], dqkv[:, :, H + Hk:], True, scale,
                     0.0, 0, 0, None, dmask, None, 0, None)
    assert bool((buf[:pad] == sentinel).all()) and bool((buf[pad + n:] == sentinel).all())
    _, _, dq, dk, dv, _ = _fwd_bwd(q.contiguous(), k.contiguous(), v.contiguous(), do, True, 0.0, None, None, 0, 0)
    assert torch.equal(dqkv[:, :, :H], dq)
    assert torch.equal(dqkv[:, :, H:H + Hk], dk)
    assert torch.equal(dqkv[:, :, H + Hk:], dv)


def test_grouped_packed_with_all_heads_equals_packed():
    from apex.contrib.multihead_attn import flash

    B, S, H, D = 2, 150, 3, 64
    base = _rand((B, S, 3 * H, D), BF, 41)
    a = base.clone().requires_grad_(True)
    b = base.clone().requires_grad_(True)
    do = _rand((B, S, H, D), BF, 42, 1.0)
    oa = flash.flash_attention_grouped_packed(a, H, H, 0.0, True)
    ob = flash.flash_attention_packed(b.view(B, S, 3, H, D), 0.0, True)
    oa.backward(do)
    ob.backward(do)
    assert torch.equal(oa, ob)
    assert torch.equal(a.grad, b.grad)


def test_grouped_refuses_dsum_and_fp8_codes():
    C = _C()
    B, S, H, Hk, D = 1, 64, 4, 2, 64
    q = _rand((B, S, H, D), BF, 51)
    k, v = _rand((B, S, Hk, D), BF, 52), _rand((B, S, Hk, D), BF, 53)
    scale = 1.0 / math.sqrt(D)
    o, lse, dmask = C.flash_attn_fwd(q, k, v, False, scale, 0.0, 0, 0, None, None)
    do = torch.ones_like(o)
    dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
    args = (do, q, k, v, o, lse, dq, dk, dv, False, scale, 0.0, 0, 0, None, dmask)
    dsum = torch.zeros(B, 3 * H * D, device=DEV)
    with pytest.raises(RuntimeError, match="grouped"):
        C.flash_attn_bwd(*args, dsum)
    cq, ck, cv = (torch.empty(t.shape, dtype=torch.uint8, device=DEV) for t in (q, k, v))
    s8, a8 = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    for only in (False, True):
        with pytest.raises(RuntimeError, match="grouped"):
            C.flash_attn_bwd(*args, None, q8_dq=cq, q8_dk=ck, q8_dv=cv, q8_scale=s8, q8_amax=a8, q8_fmt=1,
                             q8_only=only)
    with pytest.raises(RuntimeError, match="grouped"):
        C.flash_attn_bwd(*args, None, q8_only=True)
    # 3 K/V heads do not divide 4 query heads
    k3 = _rand((B, S, 3, D), BF, 54)
    with pytest.raises(RuntimeError, match="K/V heads"):
        C.flash_attn_fwd(q, k3, k3, False, scale, 0.0, 0, 0, None, None)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_rope_grouped(dtype):
    from apex.transformer.functional import fused_rope as fr

    B, S, H, Hk, d = 2, 70, 6, 2, 64
    rot = H + Hk
    gen = torch.Generator().manual_seed(3)
    ang = (torch.rand(S, d, generator=gen) * 6.0).to(DEV)
    cos, sin = ang.cos(), ang.sin()
    qkv = _rand((B, S, H + 2 * Hk, d), dtype, 61, 1.0).requires_grad_(True)
    out = fr.apply_rotary_qkv_grouped(qkv, cos, sin, H, Hk)
    assert out.shape == qkv.shape and out.is_contiguous() and out.dtype == dtype
    xr = qkv.detach().float().requires_grad_(True)
    ref = fr.rope_reference_qkv_grouped(xr, cos, sin, H, Hk)
    # the band of tests/test_fused_rope_gpu.py: fp32 math, one rounding
    rtol = 1e-5 if dtype == F32 else torch.finfo(dtype).eps
    torch.testing.assert_close(out.detach()[:, :, :rot].float(), ref.detach()[:, :, :rot], rtol=rtol, atol=1e-5)
    # Q and K separately against the plain [s, b, h, d] reference
    qk = fr.rope_reference(qkv.detach().float()[:, :, :rot].transpose(0, 1), cos, sin).transpose(0, 1)
    torch.testing.assert_close(out.detach()[:, :, :rot].float(), qk, rtol=rtol, atol=1e-5)
    assert torch.equal(out[:, :, rot:], qkv[:, :, rot:])  # V: bit-identical
    g = _rand(qkv.shape, dtype, 62, 1.0)
    (dqkv,) = torch.autograd.grad(out, qkv, g)
    (dref,) = torch.autograd.grad(ref, xr, g.float())
    torch.testing.assert_close(dqkv[:, :, :rot].float(), dref[:, :, :rot], rtol=rtol, atol=1e-5)
    assert torch.equal(dqkv[:, :, rot:], g[:, :, rot:])  # dV: bit-identical


@pytest.mark.parametrize("fused_ln", [True, False])
def test_gpt_mqa_rope_step_matches_fp32_cpu(fused_ln, monkeypatch):
    """GPTModel tiny, n_kv_head = 1, rope, bf16 on the device: loss and every parameter gradient
    against the fp32 CPU run of the same (bf16-rounded) weights, through forward_fused and forward.
    Band of tests/test_gpt_fused_gpu.py: rtol = atol = 2e-2 on the loss, relative Frobenius error
    below 2e-2 per parameter gradient."""
    from apex.models import GPTConfig, GPTModel
    from apex.models import gpt as gpt_mod

    monkeypatch.setattr(gpt_mod, "_FUSED_LN", fused_ln)
    torch.manual_seed(0)
    c = GPTConfig(vocab_size=1000, n_positions=128, n_embd=128, n_layer=2, n_head=4, n_kv_head=1, dropout=0.0,
                  position_embedding_type="rope")
    ref = GPTModel(c).to(BF).float()  # fp32 model holding bf16-representable weights
    assert ref.blocks[0].c_attn.weight.shape == ((4 + 2) * 32, 128)
    m = GPTModel(c)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).to(BF)
    ids = torch.randint(0, c.vocab_size, (2, 64))
    loss_ref = ref(ids, ids)
    loss_ref.backward()
    loss = m(ids.to(DEV), ids.to(DEV))
    loss.backward()
    print("loss", float(loss.detach()), float(loss_ref.detach()))
    torch.testing.assert_close(loss.float().cpu(), loss_ref, rtol=2e-2, atol=2e-2)
    rp = dict(ref.named_parameters())
    errs = {n: float((p.grad.float().cpu() - rp[n].grad).norm() / rp[n].grad.norm().clamp_min(1e-12))
            for n, p in m.named_parameters()}
    print({n: round(e, 5) for n, e in errs.items()})
    assert max(errs.values()) < 2e-2, errs
