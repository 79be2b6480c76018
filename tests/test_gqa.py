"""Grouped-query attention (Hk < H key/value heads), CPU tier: the attention entry points against
the reference on hand-expanded K/V, grouped RoPE, and the GPT / Megatron GPT options against MHA
models whose K/V projection rows are the group-replicated copies. fp32, assert_close defaults."""
import os
import socket
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HEADS = [(4, 2), (4, 1), (6, 2)]
B, S, D = 2, 37, 16


def _inputs(H, Hk, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, S, H, D, generator=g)
    k = torch.randn(B, S, Hk, D, generator=g)
    v = torch.randn(B, S, Hk, D, generator=g)
    do = torch.randn(B, S, H, D, generator=g)
    bias = torch.randn(1, H, S, S, generator=g) * 0.5
    return q, k, v, do, bias


def _variant(name, bias):
    kw = dict(causal=False, k_lens=None, attn_bias=None)
    if name == "causal":
        kw["causal"] = True
    elif name == "k_lens":
        kw["k_lens"] = torch.tensor([S, 11], dtype=torch.int32)
    elif name == "bias":
        kw["attn_bias"] = bias
    return kw


def _group_sum(x, g):
    b, s, h, d = x.shape
    return x.view(b, s, h // g, g, d).sum(3)


def _reference(q, k, v, do, g, kw):
    """attention_reference on hand-expanded K/V; dK/dV = the group sum of the expanded gradient."""
    from apex.contrib.multihead_attn.attention import attention_reference

    ke = k.repeat_interleave(g, dim=2).detach().requires_grad_(True)
    ve = v.repeat_interleave(g, dim=2).detach().requires_grad_(True)
    qr = q.detach().clone().requires_grad_(True)
    kw = dict(kw)
    br = kw["attn_bias"]
    if br is not None:
        br = kw["attn_bias"] = br.detach().clone().requires_grad_(True)
    o = attention_reference(qr, ke, ve, **kw)
    o.backward(do)
    return o.detach(), qr.grad, _group_sum(ke.grad, g), _group_sum(ve.grad, g), None if br is None else br.grad


@pytest.mark.parametrize("variant", ["plain", "causal", "k_lens", "bias"])
@pytest.mark.parametrize("H,Hk", HEADS)
def test_attention_grouped_matches_expanded_reference(H, Hk, variant):
    from apex.contrib.multihead_attn.attention import attention

    q, k, v, do, bias = _inputs(H, Hk)
    kw = _variant(variant, bias)
    o_ref, dq_ref, dk_ref, dv_ref, db_ref = _reference(q, k, v, do, H // Hk, kw)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    if kw["attn_bias"] is not None:
        kw["attn_bias"] = bias.clone().requires_grad_(True)
    o = attention(q, k, v, **kw)
    o.backward(do)
    assert k.grad.shape == (B, S, Hk, D) and v.grad.shape == (B, S, Hk, D)
    torch.testing.assert_close(o, o_ref)
    torch.testing.assert_close(q.grad, dq_ref)
    torch.testing.assert_close(k.grad, dk_ref)
    torch.testing.assert_close(v.grad, dv_ref)
    if db_ref is not None:
        torch.testing.assert_close(kw["attn_bias"].grad, db_ref)


@pytest.mark.parametrize("variant", ["plain", "causal", "k_lens", "bias"])
@pytest.mark.parametrize("H,Hk", HEADS)
def test_attention_grouped_packed_matches_expanded_reference(H, Hk, variant):
    from apex.contrib.multihead_attn.attention import attention_grouped_packed
    from apex.ops import fused as fops

    q, k, v, do, bias = _inputs(H, Hk, 1)
    kw = _variant(variant, bias)
    o_ref, dq_ref, dk_ref, dv_ref, db_ref = _reference(q, k, v, do, H // Hk, kw)
    qkv = torch.cat([q, k, v], 2).requires_grad_(True)
    assert qkv.shape == (B, S, H + 2 * Hk, D)
    if kw["attn_bias"] is not None:
        kw["attn_bias"] = bias.clone().requires_grad_(True)
    o = attention_grouped_packed(qkv, H, Hk, kw["attn_bias"], 0.0, kw["causal"], None, kw["k_lens"])
    o.backward(do)
    torch.testing.assert_close(o, o_ref)
    torch.testing.assert_close(qkv.grad, torch.cat([dq_ref, dk_ref, dv_ref], 2))
    if db_ref is not None:
        torch.testing.assert_close(kw["attn_bias"].grad, db_ref)
    with torch.no_grad():  # the apex.ops.fused wrapper is the same call
        assert torch.equal(fops.attention_qkv_grouped(qkv, H, Hk, kw["attn_bias"], 0.0, kw["causal"], None,
                                                      kw["k_lens"]), o)


def test_heads_must_divide():
    from apex.contrib.multihead_attn import flash
    from apex.contrib.multihead_attn.attention import attention, attention_grouped_packed, attention_reference

    q, k = torch.randn(1, 8, 4, 16), torch.randn(1, 8, 3, 16)
    with pytest.raises(ValueError, match="multiple"):
        attention(q, k, k)
    with pytest.raises(ValueError, match="multiple"):
        attention_reference(q, k, k)
    with pytest.raises(ValueError, match="multiple"):
        flash.flash_attention(q, k, k)  # raised before any launch (no device needed)
    with pytest.raises(ValueError, match="multiple"):
        attention_grouped_packed(torch.randn(1, 8, 10, 16), 4, 3)
    with pytest.raises(ValueError, match="multiple"):
        flash.flash_attention_grouped_packed(torch.randn(1, 8, 10, 16), 4, 3)
    with pytest.raises(ValueError, match="num_heads"):
        attention_grouped_packed(torch.randn(1, 8, 9, 16), 4, 2)


def test_context_parallel_refuses_grouped_heads():
    from apex.transformer import context_parallel as cp

    q, k = torch.randn(1, 8, 4, 16), torch.randn(1, 8, 2, 16)
    for fn in (cp.ring_attention, cp.ulysses_attention):
        with pytest.raises(NotImplementedError, match="grouped-query"):
            fn(q, k, k)


@pytest.mark.parametrize("H,Hk,d,d2", [(4, 2, 16, 16), (6, 1, 32, 16)])
def test_rope_grouped(H, Hk, d, d2):
    from apex.transformer.functional import apply_rotary_qkv_grouped
    from apex.transformer.functional import fused_rope as fr

    gen = torch.Generator().manual_seed(2)
    ang = torch.rand(S, d2, generator=gen) * 6.0
    cos, sin = ang.cos(), ang.sin()
    qkv = torch.randn(B, S, H + 2 * Hk, d, generator=gen).requires_grad_(True)
    out = apply_rotary_qkv_grouped(qkv, cos, sin, H, Hk)
    assert out.shape == qkv.shape
    # rope_reference on the Q and the K views separately; V passes through bit-equal
    x = qkv.detach().clone().requires_grad_(True)
    rq = fr.rope_reference(x[:, :, :H].transpose(0, 1), cos, sin).transpose(0, 1)
    rk = fr.rope_reference(x[:, :, H:H + Hk].transpose(0, 1), cos, sin).transpose(0, 1)
    torch.testing.assert_close(out[:, :, :H], rq)
    torch.testing.assert_close(out[:, :, H:H + Hk], rk)
    assert torch.equal(out[:, :, H + Hk:], qkv[:, :, H + Hk:])
    torch.testing.assert_close(fr.rope_reference_qkv_grouped(qkv, cos, sin, H, Hk), out)
    g = torch.randn(out.shape, generator=gen)
    (dx,) = torch.autograd.grad(out, qkv, g)
    (dref,) = torch.autograd.grad(torch.cat([rq, rk, x[:, :, H + Hk:]], 2), x, g)
    torch.testing.assert_close(dx, dref)
    assert torch.equal(dx[:, :, H + Hk:], g[:, :, H + Hk:])
    with pytest.raises(ValueError):
        apply_rotary_qkv_grouped(qkv, cos, sin, H, Hk + 1)


# ------------------------------------------------------------------------------------------------
# models: a GQA model equals the MHA model whose K/V projection rows are the replicated groups
# ------------------------------------------------------------------------------------------------
def _replicate_kv(t, H, Hk, d):
    """[(H + 2 Hk) d, ...] grouped projection rows (or bias) -> [3 H d, ...] MHA rows."""
    g = H // Hk
    tail = t.shape[1:]
    qr, kr, vr = t[:H * d], t[H * d:(H + Hk) * d], t[(H + Hk) * d:]
    rep = lambda x: x.reshape(Hk, d, *tail).repeat_interleave(g, dim=0).reshape(H * d, *tail)
    return torch.cat([qr, rep(kr), rep(vr)], 0)


def _fold_kv_grad(t, H, Hk, d):
    """[3 H d, ...] MHA gradient -> [(H + 2 Hk) d, ...]: K/V rows summed over each group."""
    g = H // Hk
    tail = t.shape[1:]
    qr, kr, vr = t[:H * d], t[H * d:2 * H * d], t[2 * H * d:]
    fold = lambda x: x.reshape(Hk, g, d, *tail).sum(1).reshape(Hk * d, *tail)
    return torch.cat([qr, fold(kr), fold(vr)], 0)


def _load_replicated(mha, gqa, qkv_key, H, Hk, d):
    sd = {}
    for n, t in gqa.state_dict().items():
        sd[n] = _replicate_kv(t, H, Hk, d) if qkv_key in n else t.clone()
    mha.load_state_dict(sd)


@pytest.mark.parametrize("pos", ["learned", "rope"])
@pytest.mark.parametrize("Hk", [2, 1])
@pytest.mark.parametrize("fused_ln", [True, False])
def test_gpt_gqa_equals_replicated_mha(Hk, pos, fused_ln, monkeypatch):
    from apex.models import GPTConfig, GPTModel
    from apex.models import gpt as gpt_mod

    monkeypatch.setattr(gpt_mod, "_FUSED_LN", fused_ln)
    H, E = 4, 64
    d = E // H
    kw = dict(vocab_size=200, n_positions=32, n_embd=E, n_layer=2, n_head=H, dropout=0.0, position_embedding_type=pos)
    torch.manual_seed(0)
    gqa = GPTModel(GPTConfig(n_kv_head=Hk, **kw))
    mha = GPTModel(GPTConfig(**kw))
    with torch.no_grad():
        for n, p in gqa.named_parameters():  # biases are zero-initialised: make them count
            if n.endswith("c_attn.bias"):
                p.normal_(0.0, 0.1)
    for blk in gqa.blocks:
        assert blk.c_attn.weight.shape == ((H + 2 * Hk) * d, E) and blk.c_attn.bias.shape == ((H + 2 * Hk) * d,)
        assert blk.c_proj.weight.shape == (E, E)
    _load_replicated(mha, gqa, "c_attn", H, Hk, d)
    ids = torch.randint(0, 200, (2, 19), generator=torch.Generator().manual_seed(1))
    lg, lm = gqa(ids), mha(ids)
    torch.testing.assert_close(lg, lm)
    # gradients of the training loss (the model's own shifted cross entropy)
    loss_g, loss_m = gqa(ids, ids), mha(ids, ids)
    torch.testing.assert_close(loss_g, loss_m)
    loss_g.backward()
    loss_m.backward()
    pm = dict(mha.named_parameters())
    for n, p in gqa.named_parameters():
        ref = pm[n].grad
        if "c_attn" in n:
            ref = _fold_kv_grad(ref, H, Hk, d)
        torch.testing.assert_close(p.grad, ref, msg=lambda m, n=n: f"{n}: {m}")


GPT_PARENT_SHAPES = {
    "wte.weight": (1024, 128), "wpe.weight": (128, 128), "blocks.0.ln_1.weight": (128,),
    "blocks.0.ln_1.bias": (128,), "blocks.0.c_attn.weight": (384, 128), "blocks.0.c_attn.bias": (384,),
    "blocks.0.c_proj.weight": (128, 128), "blocks.0.c_proj.bias": (128,), "blocks.0.ln_2.weight": (128,),
    "blocks.0.ln_2.bias": (128,), "blocks.0.c_fc.weight": (512, 128), "blocks.0.c_fc.bias": (512,),
    "blocks.0.mlp_proj.weight": (128, 512), "blocks.0.mlp_proj.bias": (128,), "ln_f.weight": (128,),
    "ln_f.bias": (128,)}
MEGATRON_PARENT_SHAPES = {
    "word_embeddings.weight": (512, 128), "position_embeddings.weight": (64, 128),
    "layers.0.input_layernorm.weight": (128,), "layers.0.input_layernorm.bias": (128,),
    "layers.0.query_key_value.weight": (384, 128), "layers.0.query_key_value.bias": (384,),
    "layers.0.dense.weight": (128, 128), "layers.0.dense.bias": (128,),
    "layers.0.post_attention_layernorm.weight": (128,), "layers.0.post_attention_layernorm.bias": (128,),
    "layers.0.dense_h_to_4h.weight": (512, 128), "layers.0.dense_h_to_4h.bias": (512,),
    "layers.0.dense_4h_to_h.weight": (128, 512), "layers.0.dense_4h_to_h.bias": (128,),
    "final_layernorm.weight": (128,), "final_layernorm.bias": (128,)}


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_gpt_default_is_unchanged():
    from apex.models import GPTConfig, GPTModel

    kw = dict(vocab_size=1000, n_positions=128, n_embd=128, n_layer=1, n_head=2)
    assert GPTConfig(**kw).n_kv_head is None
    for c in (GPTConfig(**kw), GPTConfig(n_kv_head=None, **kw), GPTConfig(n_kv_head=2, **kw)):
        sd = _shapes(GPTModel(c))
        assert list(sd) == list(GPT_PARENT_SHAPES) and sd == GPT_PARENT_SHAPES
    with pytest.raises(ValueError, match="n_kv_head"):
        GPTConfig(n_head=4, n_kv_head=3)
    with pytest.raises(ValueError, match="n_kv_head"):
        GPTConfig(n_head=4, n_kv_head=0)


# ---- Megatron GPT at TP = 1 (one gloo rank, the spawn pattern of tests/test_megatron_tp4pp2.py)
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _wrap(fn, rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.set_num_threads(1)
        fn(rank, world)
        q.put((rank, "ok"))
    except Exception:
        q.put((rank, traceback.format_exc()))
    finally:
        from apex.transformer import parallel_state as ps

        ps.destroy_model_parallel()
        dist.destroy_process_group()


def _spawn(fn, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_wrap, args=(fn, r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == "ok" for r in res), res


def _megatron_gqa(rank, world):
    from apex.models.megatron_gpt import MegatronGPTConfig, build_stage
    from apex.transformer import parallel_state as ps

    ps.initialize_model_parallel(1, 1)
    H, Hk, E = 4, 2, 128
    d = E // H
    kw = dict(vocab_size=512, hidden_size=E, num_attention_heads=H, max_position_embeddings=64, hidden_dropout=0.0,
              attention_dropout=0.0)

    # defaults: keys and shapes as before the option existed
    assert MegatronGPTConfig(**kw).num_query_groups is None
    for extra in ({}, {"num_query_groups": None}, {"num_query_groups": H}):
        sd = _shapes(build_stage(MegatronGPTConfig(num_layers=1, **kw, **extra)))
        assert list(sd) == list(MEGATRON_PARENT_SHAPES) and sd == MEGATRON_PARENT_SHAPES

    # config validation
    for bad in (3, 0, 8):
        try:
            MegatronGPTConfig(num_query_groups=bad, **kw)
        except ValueError as e:
            assert "num_query_groups" in str(e)
        else:
            raise AssertionError(f"num_query_groups={bad} accepted")

    for pos in ("learned", "rope"):
        torch.manual_seed(0)
        gqa = build_stage(MegatronGPTConfig(num_layers=2, num_query_groups=Hk, position_embedding_type=pos, **kw))
        mha = build_stage(MegatronGPTConfig(num_layers=2, position_embedding_type=pos, **kw))
        with torch.no_grad():
            for n, p in gqa.named_parameters():
                if n.endswith("query_key_value.bias"):
                    p.normal_(0.0, 0.1)
        for L in gqa.layers:
            assert L.query_key_value.weight.shape == ((H + 2 * Hk) * d, E)
            assert L.query_key_value.bias.shape == ((H + 2 * Hk) * d,)
        _load_replicated(mha, gqa, "query_key_value", H, Hk, d)
        ids = torch.randint(0, 512, (2, 24), generator=torch.Generator().manual_seed(7))
        with torch.no_grad():
            torch.testing.assert_close(gqa(ids), mha(ids))
        lg, lm = gqa(ids, ids), mha(ids, ids)
        torch.testing.assert_close(lg, lm)
        lg.backward()
        lm.backward()
        pm = dict(mha.named_parameters())
        for n, p in gqa.named_parameters():
            ref = pm[n].grad
            if "query_key_value" in n:
                ref = _fold_kv_grad(ref, H, Hk, d)
            torch.testing.assert_close(p.grad, ref, msg=lambda m, n=n: f"{pos} {n}: {m}")


def test_megatron_gqa_tp1():
    _spawn(_megatron_gqa, 1)
