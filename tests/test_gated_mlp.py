"""The gated MLP (SwiGLU / GEGLU) in the two GPT models, on the CPU: GPTModel against a hand-written
composition over the same weights, the default configuration's parameters unchanged, and Megatron GPT
under tensor parallelism (2 gloo ranks) against the TP = 1 model assembled from the shards."""
import math
import os
import socket
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F


# ----------------------------------------------------------------------------
# GPTModel
# ----------------------------------------------------------------------------
def _hand_gpt(m, ids, labels, act):
    """GPTModel's forward (learned positions, full multi-head attention, no dropout) in plain PyTorch."""
    c = m.config
    B, S = ids.shape
    h, d = c.n_head, c.n_embd // c.n_head
    x = m.wte.weight[ids] + m.wpe.weight[torch.arange(S)][None]
    causal = torch.ones(S, S, dtype=torch.bool).tril()
    for blk in m.blocks:
        xn = F.layer_norm(x, (c.n_embd,), blk.ln_1.weight, blk.ln_1.bias, c.layer_norm_eps)
        q, k, v = F.linear(xn, blk.c_attn.weight, blk.c_attn.bias).view(B, S, 3, h, d).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(d)
        p = s.masked_fill(~causal, float("-inf")).softmax(-1)
        ctx = (p @ v).transpose(1, 2).reshape(B, S, c.n_embd)
        x = x + F.linear(ctx, blk.c_proj.weight, blk.c_proj.bias)
        xn = F.layer_norm(x, (c.n_embd,), blk.ln_2.weight, blk.ln_2.bias, c.layer_norm_eps)
        gate, up = F.linear(xn, blk.c_fc.weight, blk.c_fc.bias).chunk(2, -1)
        x = x + F.linear(act(gate) * up, blk.mlp_proj.weight, blk.mlp_proj.bias)
    x = F.layer_norm(x, (c.n_embd,), m.ln_f.weight, m.ln_f.bias, c.layer_norm_eps)
    logits = F.linear(x, m.wte.weight)
    return F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), labels[:, 1:].reshape(-1))


@pytest.mark.parametrize("fused_ln", [True, False])
@pytest.mark.parametrize("activation", ["swiglu", "geglu"])
def test_gpt_gated_mlp_matches_hand_written(activation, fused_ln, monkeypatch):
    from apex.models import gpt
    from apex.models.gpt import GPTConfig, GPTModel

    monkeypatch.setattr(gpt, "_FUSED_LN", fused_ln)
    torch.manual_seed(0)
    c = GPTConfig(vocab_size=100, n_positions=32, n_embd=32, n_layer=2, n_head=2, dropout=0.0,
                  activation=activation, ffn_hidden_size=48)
    m = GPTModel(c)
    blk = m.blocks[0]
    assert blk.c_fc.weight.shape == (96, 32) and blk.c_fc.bias.shape == (96,) and blk.mlp_proj.weight.shape == (32, 48)
    # the GPT-2 scaled init reaches the gated block's output projection
    assert float(blk.mlp_proj.weight.detach().std()) < 0.75 * float(blk.c_fc.weight.detach().std())
    with torch.no_grad():   # zero-initialised biases would hide a misplaced one
        for n, p in m.named_parameters():
            if p.ndim == 1:
                p.add_(torch.randn(p.shape) * 0.05)
    ids = torch.randint(0, c.vocab_size, (2, 16), generator=torch.Generator().manual_seed(1))
    loss = m(ids, ids)
    loss.backward()
    got = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    act = F.silu if activation == "swiglu" else (lambda t: F.gelu(t, approximate="tanh"))
    want = _hand_gpt(m, ids, ids, act)
    want.backward()
    # fp32 on both sides; the two differ in the order of their fp32 operations only
    torch.testing.assert_close(loss.detach(), want.detach(), rtol=1e-5, atol=1e-6)
    for n, p in m.named_parameters():
        torch.testing.assert_close(got[n], p.grad, rtol=1e-4, atol=1e-6, msg=lambda s, n=n: f"{n}: {s}")
    assert float(got["blocks.0.c_fc.bias"].abs().max()) > 0


def test_gpt_bad_activation_raises():
    from apex.models.gpt import GPTConfig
    from apex.models.megatron_gpt import MegatronGPTConfig

    with pytest.raises(ValueError, match="activation"):
        GPTConfig(activation="relu")
    with pytest.raises(ValueError, match="activation"):
        MegatronGPTConfig(activation="glu")


def test_gpt_default_parameters_unchanged():
    from apex.models.gpt import GPTConfig, GPTModel

    c = GPTConfig(vocab_size=1000, n_positions=128, n_embd=128, n_layer=2, n_head=2)
    assert c.activation == "gelu" and c.ffn_hidden_size is None
    want = [("wte.weight", (1024, 128)), ("wpe.weight", (128, 128))]
    for i in range(2):
        want += [(f"blocks.{i}.ln_1.weight", (128,)), (f"blocks.{i}.ln_1.bias", (128,)),
                 (f"blocks.{i}.c_attn.weight", (384, 128)), (f"blocks.{i}.c_attn.bias", (384,)),
                 (f"blocks.{i}.c_proj.weight", (128, 128)), (f"blocks.{i}.c_proj.bias", (128,)),
                 (f"blocks.{i}.ln_2.weight", (128,)), (f"blocks.{i}.ln_2.bias", (128,)),
                 (f"blocks.{i}.c_fc.weight", (512, 128)), (f"blocks.{i}.c_fc.bias", (512,)),
                 (f"blocks.{i}.mlp_proj.weight", (128, 512)), (f"blocks.{i}.mlp_proj.bias", (128,))]
    want += [("ln_f.weight", (128,)), ("ln_f.bias", (128,))]
    got = [(k, tuple(v.shape)) for k, v in GPTModel(c).state_dict().items()]
    assert got == want
    # a plain MLP of another width
    m = GPTModel(GPTConfig(vocab_size=100, n_positions=32, n_embd=32, n_layer=1, n_head=2, ffn_hidden_size=40))
    assert m.blocks[0].c_fc.weight.shape == (40, 32) and m.blocks[0].mlp_proj.weight.shape == (32, 40)


# ----------------------------------------------------------------------------
# Megatron GPT, TP = 2 on gloo (the pattern of tests/test_gqa_tp.py)
# ----------------------------------------------------------------------------
TP = 2
E, FFN = 64, 96


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(fn, world, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_wrap, args=(fn, r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == "ok" for r in res), res


def _wrap(fn, rank, world, port, q, *args):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.set_num_threads(1)
        fn(rank, world, *args)
        q.put((rank, "ok"))
    except Exception:
        q.put((rank, traceback.format_exc()))
    finally:
        from apex.transformer import parallel_state as ps

        ps.destroy_model_parallel()
        dist.destroy_process_group()


def _gather(t):
    from apex.transformer import parallel_state as ps

    parts = [torch.empty_like(t) for _ in range(TP)]
    dist.all_gather(parts, t.detach().contiguous(), group=ps.get_tensor_model_parallel_group())
    return parts


def _full(name, t):
    """A parameter (or gradient) of the TP = 2 model in the TP = 1 layout."""
    if "dense_h_to_4h" in name:
        # shards [gate_r; up_r] of every rank -> [cat(gate_r); cat(up_r)] (weight rows and bias alike)
        parts = _gather(t)
        fl = FFN // TP
        return torch.cat([p[:fl] for p in parts] + [p[fl:] for p in parts], 0)
    if name.endswith("dense.weight") or name.endswith("dense_4h_to_h.weight"):
        return torch.cat(_gather(t), 1)
    if "query_key_value" in name:
        # [3, heads_local, d] per rank -> [3, heads, d]
        parts = [p.view(3, -1, *p.shape[1:]) for p in _gather(t)]
        return torch.cat(parts, 1).reshape(-1, *t.shape[1:])
    if "word_embeddings" in name:
        return torch.cat(_gather(t), 0)
    return t.detach().clone()


def _tp2_vs_tp1(rank, world, activation):
    from apex.models.megatron_gpt import MegatronGPTConfig, build_stage
    from apex.transformer import parallel_state as ps

    def cfg(ffn=FFN):
        return MegatronGPTConfig(vocab_size=128, hidden_size=E, num_layers=2, num_attention_heads=4,
                                 ffn_hidden_size=ffn, max_position_embeddings=32, hidden_dropout=0.0,
                                 attention_dropout=0.0, activation=activation)

    ps.initialize_model_parallel(TP, 1)
    torch.manual_seed(100 + rank)  # every shard different; replicated parameters synced below
    m2 = build_stage(cfg())
    f1, f2 = m2.layers[0].dense_h_to_4h, m2.layers[0].dense_4h_to_h
    assert f1.weight.shape == (2 * FFN // TP, E) and f1.bias.shape == (2 * FFN // TP,)
    assert f2.weight.shape == (E, FFN // TP)
    with torch.no_grad():
        for n, p in m2.named_parameters():
            if p.ndim == 1:
                p.add_(torch.randn(p.shape) * 0.05)
    src, grp = ps.get_tensor_model_parallel_src_rank(), ps.get_tensor_model_parallel_group()
    for n, p in m2.named_parameters():
        if not getattr(p, "tensor_model_parallel", False):
            dist.broadcast(p.data, src, group=grp)
    ids = torch.randint(0, 128, (2, 24), generator=torch.Generator().manual_seed(3))
    loss2 = m2(ids, ids)
    loss2.backward()
    weights = {n: _full(n, p) for n, p in m2.named_parameters()}
    grads = {n: _full(n, p.grad) for n, p in m2.named_parameters()}

    # the MLP width must divide over the TP ranks
    try:
        build_stage(cfg(ffn=95))
    except ValueError as e:
        assert "ffn_hidden_size" in str(e)
    else:
        raise AssertionError("ffn_hidden_size=95 accepted at TP=2")

    ps.destroy_model_parallel()
    ps.initialize_model_parallel(1, 1)
    m1 = build_stage(cfg())
    assert m1.layers[0].dense_h_to_4h.weight.shape == (2 * FFN, E)
    m1.load_state_dict(weights)
    loss1 = m1(ids, ids)
    loss1.backward()
    torch.testing.assert_close(loss2.detach(), loss1.detach(), rtol=1e-5, atol=1e-6)
    for n, p in m1.named_parameters():
        # the band tests/test_megatron_tp4pp2.py uses for sharded against serial gradients
        torch.testing.assert_close(grads[n], p.grad, rtol=2e-4, atol=2e-5, msg=lambda m, n=n: f"{n}: {m}")
    for n in ("layers.0.dense_h_to_4h.weight", "layers.0.dense_h_to_4h.bias"):
        assert float(grads[n].abs().max()) > 0

    # the TP = 1 gated MLP is the hand-written composition over its weights
    lay = m1.layers[0]
    x = torch.randn(2, 5, E, generator=torch.Generator().manual_seed(4))
    out, bias = lay._gated_mlp(x)
    gate, up = F.linear(x, lay.dense_h_to_4h.weight, lay.dense_h_to_4h.bias).chunk(2, -1)
    act = F.silu if activation == "swiglu" else F.gelu   # Megatron's geglu: erf
    want = F.linear(act(gate) * up, lay.dense_4h_to_h.weight, lay.dense_4h_to_h.bias)
    torch.testing.assert_close(out + bias, want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("activation", ["swiglu", "geglu"])
def test_megatron_gated_mlp_tp2_matches_tp1(activation):
    _spawn(_tp2_vs_tp1, TP, activation)
