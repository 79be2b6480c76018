"""Grouped-query Megatron GPT under tensor parallelism (2 gloo ranks on the CPU): TP = 2, 2 layers,
hidden 64, 4 heads in 2 query groups. Each rank's query_key_value shard is laid out rank-locally as
its Q heads, K heads, V heads; the loss and the gathered QKV weight gradient must equal those of the
TP = 1 model whose QKV weight is assembled from the shards as cat(q_r), cat(k_r), cat(v_r)."""
import os
import socket
import traceback

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

TP = 2
H, HK, E = 4, 2, 64
D = E // H


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


def _qkv_full(t):
    """Shards [(h_local + 2 hk_local) d, ...] of every rank -> the TP = 1 rows cat(q_r), cat(k_r), cat(v_r)."""
    hl, kl = H // TP, HK // TP
    parts = _gather(t)
    q = [p[:hl * D] for p in parts]
    k = [p[hl * D:(hl + kl) * D] for p in parts]
    v = [p[(hl + kl) * D:] for p in parts]
    return torch.cat(q + k + v, 0)


def _full(name, t):
    """A parameter (or gradient) of the TP = 2 model in the TP = 1 layout."""
    if "query_key_value" in name:
        return _qkv_full(t)
    if name.endswith("dense.weight") or name.endswith("dense_4h_to_h.weight"):
        return torch.cat(_gather(t), 1)
    if "dense_h_to_4h" in name or "word_embeddings" in name:
        return torch.cat(_gather(t), 0)
    return t.detach().clone()


def _tp2_vs_tp1(rank, world):
    from apex.models.megatron_gpt import MegatronGPTConfig, build_stage
    from apex.transformer import parallel_state as ps

    def cfg():
        return MegatronGPTConfig(vocab_size=128, hidden_size=E, num_layers=2, num_attention_heads=H,
                                 num_query_groups=HK, max_position_embeddings=32, hidden_dropout=0.0,
                                 attention_dropout=0.0, position_embedding_type="rope")

    ps.initialize_model_parallel(TP, 1)
    torch.manual_seed(100 + rank)  # every shard different; replicated parameters synced below
    m2 = build_stage(cfg())
    assert m2.layers[0].query_key_value.weight.shape == ((H + 2 * HK) * D // TP, E)
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

    # the query groups must divide over the TP ranks
    try:
        build_stage(MegatronGPTConfig(vocab_size=128, hidden_size=E, num_layers=1, num_attention_heads=H,
                                      num_query_groups=1, max_position_embeddings=32))
    except ValueError as e:
        assert "num_query_groups" in str(e)
    else:
        raise AssertionError("num_query_groups=1 accepted at TP=2")

    ps.destroy_model_parallel()
    ps.initialize_model_parallel(1, 1)
    m1 = build_stage(cfg())
    m1.load_state_dict(weights)
    loss1 = m1(ids, ids)
    loss1.backward()
    torch.testing.assert_close(loss2.detach(), loss1.detach(), rtol=1e-5, atol=1e-6)
    for n, p in m1.named_parameters():
        # the band tests/test_megatron_tp4pp2.py uses for sharded against serial gradients
        torch.testing.assert_close(grads[n], p.grad, rtol=2e-4, atol=2e-5, msg=lambda m, n=n: f"{n}: {m}")
    assert float(grads["layers.0.query_key_value.weight"].abs().max()) > 0


def test_megatron_gqa_tp2_matches_tp1():
    _spawn(_tp2_vs_tp1, TP)
