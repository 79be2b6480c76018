"""Fused rotary position embedding, CPU tier: the PyTorch reference path of
apex.transformer.functional.fused_rope (API, autograd, thd and packed forms, RotaryEmbedding) and
the ``position_embedding_type="rope"`` option of the GPT models."""
import dataclasses

import pytest
import torch

from test_transformer import _spawn

CU = [0, 5, 5, 37, 64]  # one empty sequence; T = 70 leaves six trailing tokens


def _fr():
    from apex.transformer.functional import fused_rope

    return fused_rope


def _tables(S, d2, seed=0):
    """Random angles with two DIFFERENT halves (nothing may assume cat(f, f))."""
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(S, d2, generator=g) * 6.0
    return ang


def test_exports():
    import apex.transformer.functional as F

    for n in ("fused_apply_rotary_pos_emb", "fused_apply_rotary_pos_emb_cached", "fused_apply_rotary_pos_emb_thd",
              "apply_rotary_qkv_packed", "RotaryEmbedding"):
        assert hasattr(F, n), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_api_shapes_dtypes(dtype):
    fr = _fr()
    S, B, H, D, d2 = 7, 2, 3, 12, 8
    ang = _tables(S, d2)
    t = torch.randn(S, B, H, D).to(dtype)
    y = fr.fused_apply_rotary_pos_emb(t, ang[:, None, None, :])
    assert y.shape == t.shape and y.dtype == dtype and y.is_contiguous()
    yc = fr.fused_apply_rotary_pos_emb_cached(t, ang.cos()[:, None, None, :], ang.sin()[:, None, None, :])
    assert torch.equal(y, yc)
    assert torch.equal(y[..., d2:], t[..., d2:])
    # explicit formula with distinct table halves
    c, s, x, h = ang.cos()[:, None, None], ang.sin()[:, None, None], t.float(), d2 // 2
    lo = x[..., :h] * c[..., :h] - x[..., h:d2] * s[..., :h]
    hi = x[..., h:d2] * c[..., h:] + x[..., :h] * s[..., h:]
    torch.testing.assert_close(y[..., :d2].float(), torch.cat([lo, hi], -1).to(dtype).float(), rtol=0, atol=0)
    t3 = torch.randn(11, H, D).to(dtype)
    y3 = fr.fused_apply_rotary_pos_emb_thd(t3, torch.tensor([0, 4, 11], dtype=torch.int32), ang[:, None, None, :])
    assert y3.shape == t3.shape and y3.dtype == dtype
    qkv = torch.randn(B, S, 3, H, D).to(dtype)
    yp = fr.apply_rotary_qkv_packed(qkv, ang.cos(), ang.sin())
    assert yp.shape == qkv.shape and yp.dtype == dtype and yp.is_contiguous()


def test_argument_errors():
    fr = _fr()
    t = torch.randn(8, 2, 3, 12)
    f = lambda S, d2: _tables(S, d2)[:, None, None, :]
    with pytest.raises(ValueError):
        fr.fused_apply_rotary_pos_emb(t, f(7, 8))  # table shorter than the sequence
    with pytest.raises(ValueError):
        fr.fused_apply_rotary_pos_emb(t, f(8, 7))  # odd d2
    with pytest.raises(ValueError):
        fr.fused_apply_rotary_pos_emb(t, f(8, 14))  # d2 > d
    with pytest.raises(ValueError):
        fr.apply_rotary_qkv_packed(torch.randn(2, 8, 3, 2, 12), _tables(7, 8).cos(), _tables(7, 8).sin())
    with pytest.raises(ValueError):
        fr.fused_apply_rotary_pos_emb_thd(torch.randn(8, 3, 12), torch.tensor([0, 8], dtype=torch.int32), f(8, 14))
    with pytest.raises(TypeError):
        fr.fused_apply_rotary_pos_emb(torch.zeros(8, 2, 3, 12, dtype=torch.int32), f(8, 8))
    with pytest.raises(TypeError):
        fr.apply_rotary_qkv_packed(torch.zeros(2, 8, 3, 2, 12, dtype=torch.int64), _tables(8, 8).cos(),
                                   _tables(8, 8).sin())


def test_no_grad_for_tables_and_nothing_but_tables_saved():
    fr = _fr()
    ang = _tables(6, 8).requires_grad_(True)
    t = torch.randn(6, 1, 2, 8, requires_grad=True)
    y = fr.fused_apply_rotary_pos_emb(t, ang[:, None, None, :])
    saved = y.grad_fn.saved_tensors
    assert all(s.shape == (6, 8) for s in saved), [s.shape for s in saved]
    y.sum().backward()
    assert ang.grad is None and t.grad is not None
    c, s = ang.detach().cos().requires_grad_(True), ang.detach().sin().requires_grad_(True)
    fr.fused_apply_rotary_pos_emb_cached(t, c, s).sum().backward()
    assert c.grad is None and s.grad is None


def test_gradcheck_sbhd_thd_packed():
    fr = _fr()
    ang = _tables(9, 6)
    f = ang[:, None, None, :]
    t = torch.randn(9, 2, 3, 10, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x: fr.fused_apply_rotary_pos_emb(x, f), (t,))
    assert torch.autograd.gradcheck(lambda x: fr.fused_apply_rotary_pos_emb(x, f, True), (t,))
    cu = torch.tensor([0, 3, 3, 9, 12], dtype=torch.int32)
    t3 = torch.randn(14, 2, 10, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x: fr.fused_apply_rotary_pos_emb_thd(x, cu, f), (t3,))
    q = torch.randn(2, 9, 3, 2, 10, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x: fr.apply_rotary_qkv_packed(x, ang.cos(), ang.sin()), (q,))


def test_backward_matches_autograd_through_reference():
    fr = _fr()
    ang = _tables(9, 6)
    t = torch.randn(9, 2, 3, 10, requires_grad=True)
    g = torch.randn(9, 2, 3, 10)
    (dx,) = torch.autograd.grad(fr.fused_apply_rotary_pos_emb(t, ang[:, None, None, :]), t, g)
    (dr,) = torch.autograd.grad(fr.rope_reference(t, ang.cos(), ang.sin()), t, g)
    torch.testing.assert_close(dx, dr, rtol=1e-6, atol=1e-6)


def test_transpose_output_memory():
    fr = _fr()
    S, B, H, D = 6, 3, 2, 8
    f = _tables(S, D)[:, None, None, :]
    t = torch.randn(S, B, H, D, requires_grad=True)
    y = fr.fused_apply_rotary_pos_emb(t, f)
    yt = fr.fused_apply_rotary_pos_emb(t, f, transpose_output_memory=True)
    assert yt.shape == (S, B, H, D)
    assert yt.stride() == torch.empty(B, S, H, D).transpose(0, 1).stride()
    assert torch.equal(y, yt)
    g = torch.randn(S, B, H, D)
    assert torch.equal(torch.autograd.grad(y, t, g)[0], torch.autograd.grad(yt, t, g)[0])


def test_thd_matches_per_sequence_sbhd():
    fr = _fr()
    T, H, D, d2 = 70, 2, 16, 12
    f = _tables(40, d2)[:, None, None, :]
    t = torch.randn(T, H, D)
    y = fr.fused_apply_rotary_pos_emb_thd(t, torch.tensor(CU, dtype=torch.int32), f)
    for a, b in zip(CU[:-1], CU[1:]):
        if b > a:
            ref = fr.fused_apply_rotary_pos_emb(t[a:b].unsqueeze(1), f[:b - a]).squeeze(1)
            assert torch.equal(y[a:b], ref), (a, b)
    assert torch.equal(y[CU[-1]:], t[CU[-1]:])  # six trailing tokens: bit-identical copies
    assert T - CU[-1] == 6
    # int64 cu_seqlens are accepted as well
    y64 = fr.fused_apply_rotary_pos_emb_thd(t, torch.tensor(CU), f)
    assert torch.equal(y, y64)


def test_packed_matches_sbhd_on_q_and_k():
    fr = _fr()
    B, S, h, d, d2 = 2, 9, 3, 16, 12
    ang = _tables(S, d2)
    qkv = torch.randn(B, S, 3, h, d, requires_grad=True)
    out = fr.apply_rotary_qkv_packed(qkv, ang.cos(), ang.sin())
    for i in range(2):
        ref = fr.fused_apply_rotary_pos_emb(qkv[:, :, i].transpose(0, 1), ang[:, None, None, :]).transpose(0, 1)
        assert torch.equal(out[:, :, i], ref)
    assert torch.equal(out[:, :, 2], qkv[:, :, 2])
    g = torch.randn_like(out)
    (dqkv,) = torch.autograd.grad(out, qkv, g, retain_graph=True)
    assert torch.equal(dqkv[:, :, 2], g[:, :, 2])
    (dref,) = torch.autograd.grad(fr.rope_reference_qkv_packed(qkv, ang.cos(), ang.sin()), qkv, g)
    torch.testing.assert_close(dqkv, dref, rtol=1e-6, atol=1e-6)
    # a shared (expanded) incoming gradient is read, not written
    shared = torch.randn(1, 1, 1, 1, d).expand(B, S, 3, h, d)
    keep = shared.clone()
    torch.autograd.grad(out, qkv, shared)
    assert torch.equal(shared, keep)


def test_rotary_embedding_module():
    fr = _fr()
    rot = fr.RotaryEmbedding(16)
    f = rot(10)
    assert f.shape == (10, 1, 1, 16) and f.dtype == torch.float32
    inv = 1.0 / (10000 ** (torch.arange(0, 16, 2, dtype=torch.float32) / 16))
    ref = torch.outer(torch.arange(10, dtype=torch.float32), inv)
    assert torch.equal(f[:, 0, 0], torch.cat([ref, ref], -1))
    # offset shifts positions
    assert torch.equal(rot(4, offset=6), rot(10)[6:])
    # the interpolation factor divides positions
    assert torch.allclose(fr.RotaryEmbedding(16, seq_len_interpolation_factor=4.0)(9)[8], rot(3)[2], rtol=1e-6, atol=0)
    # rotary_percent = 0.5: the first half of the head dim only
    half = fr.RotaryEmbedding(16, rotary_percent=0.5)
    assert half(5).shape == (5, 1, 1, 8)
    t = torch.randn(5, 1, 2, 16)
    y = fr.fused_apply_rotary_pos_emb(t, half(5))
    assert torch.equal(y[..., 8:], t[..., 8:]) and not torch.equal(y[1:, ..., :8], t[1:, ..., :8])
    c, s = rot.cos_sin(10)
    assert c.shape == (10, 16) and c.dtype == torch.float32
    assert torch.equal(c, rot(10)[:, 0, 0].cos()) and torch.equal(s, rot(10)[:, 0, 0].sin())
    assert rot.cos_sin(10)[0] is c  # cached
    assert rot.cos_sin(12)[0].shape == (12, 16)  # rebuilt when the length changes


def test_rotary_embedding_survives_module_cast():
    fr = _fr()

    class Owner(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(4, 4)
            self.rot = fr.RotaryEmbedding(8)

    m = Owner()
    m.rot.cos_sin(6)
    m = m.to(torch.bfloat16)
    assert m.lin.weight.dtype == torch.bfloat16
    c, s = m.rot.cos_sin(6)
    assert c.dtype == s.dtype == m.rot(6).dtype == m.rot.inv_freq.dtype == torch.float32
    assert set(m.state_dict()) == {"lin.weight", "lin.bias"}


def test_relative_position_property():
    """Scores of rotated q, k depend on relative positions only: offset 0 and offset 37 agree to
    1e-4 x max|score| (fp32 tables; measured 3.8e-6 against scores up to 16 at D = 32, S = 8)."""
    fr = _fr()
    torch.manual_seed(0)
    S, D = 8, 32
    rot = fr.RotaryEmbedding(D)
    q, k = torch.randn(S, 1, 1, D), torch.randn(S, 1, 1, D)

    def scores(offset):
        f = rot(S, offset=offset).clone()
        a = fr.fused_apply_rotary_pos_emb(q, f)[:, 0, 0]
        b = fr.fused_apply_rotary_pos_emb(k, f)[:, 0, 0]
        return a @ b.t()

    s0, s37 = scores(0), scores(37)
    err = float((s0 - s37).abs().max())
    print("relative-position error", err, "max score", float(s0.abs().max()))
    assert err <= 1e-4 * float(s0.abs().max())


# --------------------------------------------------------------------------------------------
# models
# --------------------------------------------------------------------------------------------
def _gpt(rope, **kw):
    from apex.models import GPTConfig, GPTModel

    torch.manual_seed(0)
    c = GPTConfig.tiny()
    c.dropout = 0.0
    if rope:
        c.position_embedding_type = "rope"
    for k, v in kw.items():
        setattr(c, k, v)
    return c, GPTModel(c)


def test_gpt_rope_model(monkeypatch):
    fr = _fr()
    c, m = _gpt(True)
    assert not any("wpe" in k or "rotary" in k for k in m.state_dict())
    ids = torch.randint(0, c.vocab_size, (2, 16), generator=torch.Generator().manual_seed(1))
    loss = m(ids, ids)
    loss.backward()
    assert torch.isfinite(loss)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    grads = [p.grad.clone() for p in m.parameters()]
    # the same model with the rotation done by the eager composition
    calls = []
    monkeypatch.setattr(fr, "apply_rotary_qkv_packed",
                        lambda qkv, cos, sin: (calls.append(1), fr.rope_reference_qkv_packed(qkv, cos, sin))[1])
    m.zero_grad(set_to_none=True)
    ref = m(ids, ids)
    ref.backward()
    assert len(calls) == c.n_layer
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-5)
    for g, p in zip(grads, m.parameters()):
        torch.testing.assert_close(g, p.grad, rtol=1e-4, atol=1e-6)
    # positions matter: a permuted prefix changes the logits of the last token
    with torch.no_grad():
        a = m(ids)[:, -1]
        b = m(torch.cat([ids[:, :-1].flip(1), ids[:, -1:]], 1))[:, -1]
    assert not torch.allclose(a, b)
    # no length limit from n_positions
    with torch.no_grad():
        assert m(torch.randint(0, c.vocab_size, (1, c.n_positions + 8))).shape[1] == c.n_positions + 8


def test_gpt_learned_is_unchanged():
    from apex.models import GPTConfig, GPTModel

    torch.manual_seed(0)
    base = GPTConfig(vocab_size=1000, n_positions=128, n_embd=128, n_layer=2, n_head=2, dropout=0.0)
    m0 = GPTModel(base)
    c, m1 = _gpt(False)
    assert dataclasses.asdict(c)["position_embedding_type"] == "learned"
    assert list(m0.state_dict()) == list(m1.state_dict()) and "wpe.weight" in m1.state_dict()
    ids = torch.randint(0, 1000, (2, 16), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert torch.equal(m0(ids), m1(ids))
    with pytest.raises(ValueError):
        GPTConfig(position_embedding_type="alibi")


def _megatron_rope(rank, world):
    from apex.models.megatron_gpt import MegatronGPT, MegatronGPTConfig, build_stage
    from apex.transformer import parallel_state as ps
    from apex.transformer.functional import fused_rope as fr

    ps.initialize_model_parallel(1, 1)
    ids = torch.randint(0, 512, (2, 32), generator=torch.Generator().manual_seed(7))

    # "learned": keys and seeded forward equal those of a config built without the new fields
    def learned(**kw):
        c = MegatronGPTConfig(vocab_size=512, hidden_size=128, num_layers=4, num_attention_heads=4,
                              max_position_embeddings=64, hidden_dropout=0.0, attention_dropout=0.0, **kw)
        torch.manual_seed(0)
        return build_stage(c)

    m0, m1 = learned(), learned(position_embedding_type="learned", rotary_percent=1.0, rotary_base=10000)
    assert list(m0.state_dict()) == list(m1.state_dict()) and "position_embeddings.weight" in m1.state_dict()
    with torch.no_grad():
        assert torch.equal(m0(ids), m1(ids))

    c = MegatronGPTConfig.tiny()
    c.hidden_dropout = c.attention_dropout = 0.0
    c.position_embedding_type = "rope"
    torch.manual_seed(0)
    m = build_stage(c)
    assert not any("position_embeddings" in k or "rotary" in k for k in m.state_dict())
    loss = m(ids, ids)
    loss.backward()
    assert torch.isfinite(loss)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    # a later pipeline stage owns its own RotaryEmbedding and no position table
    later = MegatronGPT(c, pre_process=False, post_process=True, layer_offset=2, num_local_layers=2)
    assert hasattr(later, "rotary_pos_emb") and not hasattr(later, "position_embeddings")
    # no length limit from max_position_embeddings
    with torch.no_grad():
        assert m(torch.randint(0, 512, (1, 72))).shape[1] == 72
    calls = []
    orig = fr.apply_rotary_qkv_packed
    fr.apply_rotary_qkv_packed = lambda qkv, cos, sin: (calls.append(1), fr.rope_reference_qkv_packed(qkv, cos, sin))[1]
    try:
        m.zero_grad(set_to_none=True)
        ref = m(ids, ids)
    finally:
        fr.apply_rotary_qkv_packed = orig
    assert len(calls) == c.num_layers
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-5)


def test_megatron_rope_model():
    _spawn(_megatron_rope, 1)
