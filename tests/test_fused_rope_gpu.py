"""Fused rotary position embedding on the GPU (csrc/rope.hip) against the PyTorch reference
composition of apex.transformer.functional.fused_rope.

Tolerance: the kernel computes in fp32 and rounds once, so it differs from the fp32 reference by at
most half an ulp of the output plus fp32 noise: rtol = eps(dtype) (2x the rounding bound eps / 2),
atol = 1e-5; fp32 uses rtol = 1e-5. Gradients follow the same rule against autograd through the
reference on fp32 copies of the same rounded inputs."""
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CU = [0, 5, 5, 37, 64]


def _fr():
    from apex.transformer.functional import fused_rope

    return fused_rope


def _close(out, ref, dtype):
    assert out.dtype == dtype
    rtol = 1e-5 if dtype == torch.float32 else torch.finfo(dtype).eps
    torch.testing.assert_close(out.float(), ref, rtol=rtol, atol=1e-5)


def _angles(S, d2, seed=0):
    """Random angles whose two halves differ (nothing may assume cat(f, f))."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(S, d2, device=DEV, generator=g) * 6.0


def _rand(shape, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, device=DEV, generator=g).to(dtype)


def _path(t4, cos, sin):
    """Which kernel the host dispatch picks for this view (1: 16-byte kernel, 0: scalar)."""
    import apex

    return apex._ext.require().rope(t4, torch.empty(t4.shape, dtype=t4.dtype, device=DEV), cos.contiguous(),
                                    sin.contiguous())


def _fwd_bwd_vs_reference(t, cos, sin, dtype, transpose_output_memory=False):
    """t: an [S, B, H, D] device view (any strides). Returns the fused output."""
    fr = _fr()
    x = t.detach().requires_grad_(True)
    y = fr.fused_apply_rotary_pos_emb_cached(x, cos, sin, transpose_output_memory)
    g = _rand(tuple(t.shape), dtype, 99)
    (dx,) = torch.autograd.grad(y, x, g)
    xr = t.detach().float().requires_grad_(True)
    yr = fr.rope_reference(xr, cos.float(), sin.float())
    (dr,) = torch.autograd.grad(yr, xr, g.float())
    _close(y.detach(), yr.detach(), dtype)
    _close(dx, dr, dtype)
    d2 = cos.shape[-1]
    assert torch.equal(y[..., d2:], t[..., d2:]) and torch.equal(dx[..., d2:], g[..., d2:])
    return y


@pytest.mark.parametrize("table_in_dtype", [False, True])
@pytest.mark.parametrize("shape", [(37, 2, 3, 64, 64), (37, 2, 3, 128, 64), (5, 1, 1, 32, 16),
                                   (130, 1, 5, 256, 256), (37, 2, 3, 80, 48)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fast_path(dtype, shape, table_in_dtype):
    """80 / 48 puts the partner chunk at a 48-byte offset (16-bit dtypes)."""
    S, B, H, D, d2 = shape
    ang = _angles(S, d2)
    cos, sin = ang.cos(), ang.sin()
    if table_in_dtype:
        cos, sin = cos.to(dtype), sin.to(dtype)
    t = _rand((S, B, H, D), dtype, 1)
    assert _path(t, cos, sin) == 1
    _fwd_bwd_vs_reference(t, cos, sin, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scalar_path(dtype):
    S, B, H, D, d2 = 9, 2, 3, 20, 10
    ang = _angles(S, d2)
    t = _rand((S, B, H, D), dtype, 2)
    assert _path(t, ang.cos(), ang.sin()) == 0
    _fwd_bwd_vs_reference(t, ang.cos(), ang.sin(), dtype)
    # a fast-path shape viewed from storage offset 1: base pointer not 16-byte aligned
    S, B, H, D, d2 = 37, 2, 3, 64, 64
    ang = _angles(S, d2)
    buf = _rand((S * B * H * D + 1,), dtype, 3)
    t = buf[1:].view(S, B, H, D)
    assert t.storage_offset() == 1 and _path(t, ang.cos(), ang.sin()) == 0
    _fwd_bwd_vs_reference(t, ang.cos(), ang.sin(), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_inputs(dtype):
    fr = _fr()
    S, B, H, D = 37, 2, 3, 64
    ang = _angles(S, D)
    cos, sin = ang.cos(), ang.sin()
    # a transposed view of [B, S, H, D]
    t = _rand((B, S, H, D), dtype, 4).transpose(0, 1)
    assert not t.is_contiguous() and _path(t, cos, sin) == 1
    y = _fwd_bwd_vs_reference(t, cos, sin, dtype)
    assert y.is_contiguous()
    # the Q slice of a packed [B, S, 3, h, d] tensor
    qkv = _rand((B, S, 3, H, D), dtype, 5)
    q = qkv[:, :, 0].transpose(0, 1)
    assert q.stride() == (3 * H * D, S * 3 * H * D, D, 1) and _path(q, cos, sin) == 1
    yq = _fwd_bwd_vs_reference(q, cos, sin, dtype)
    assert torch.equal(yq, fr.fused_apply_rotary_pos_emb_cached(q.contiguous(), cos, sin))
    # transposed output memory
    yt = _fwd_bwd_vs_reference(t, cos, sin, dtype, transpose_output_memory=True)
    assert yt.shape == (S, B, H, D) and yt.stride() == torch.empty(B, S, H, D).transpose(0, 1).stride()
    assert torch.equal(yt, y)


def test_output_must_not_alias_input():
    import apex

    ang = _angles(8, 16)
    t = _rand((8, 1, 2, 16), torch.bfloat16, 6)
    with pytest.raises(RuntimeError, match="alias"):
        apex._ext.require().rope(t, t, ang.cos(), ang.sin())
    with pytest.raises(TypeError):
        _fr().fused_apply_rotary_pos_emb_cached(t.double(), ang.cos(), ang.sin())


@pytest.mark.parametrize("shape", [(2, 37, 3, 3, 64), (1, 130, 3, 2, 128)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_packed_qkv_into_attention(dtype, shape):
    from apex.ops import fused as fops

    fr = _fr()
    B, S, _, h, d = shape
    ang = _angles(S, d)
    cos, sin = ang.cos(), ang.sin()
    qkv = _rand(shape, dtype, 7).requires_grad_(True)
    out = fr.apply_rotary_qkv_packed(qkv, cos, sin)
    assert out.shape == qkv.shape and out.is_contiguous()
    xr = qkv.detach().float().requires_grad_(True)
    ref = fr.rope_reference_qkv_packed(xr, cos, sin)
    _close(out.detach()[:, :, :2], ref.detach()[:, :, :2], dtype)
    assert torch.equal(out[:, :, 2], qkv[:, :, 2])  # V: bit-identical
    g = _rand(shape, dtype, 8)
    (dqkv,) = torch.autograd.grad(out, qkv, g, retain_graph=True)
    (dref,) = torch.autograd.grad(ref, xr, g.float())
    _close(dqkv[:, :, :2], dref[:, :, :2], dtype)
    assert torch.equal(dqkv[:, :, 2], g[:, :, 2])  # dV: bit-identical
    # end to end through the causal flash kernel
    ctx = fops.attention_qkv_packed(out, None, 0.0, causal=True)
    ctx.float().square().mean().backward()
    assert torch.isfinite(ctx.float()).all() and torch.isfinite(qkv.grad.float()).all()
    assert float(qkv.grad.float().abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_thd(dtype):
    fr = _fr()
    T, h, d = 70, 3, 64
    cu = torch.tensor(CU, dtype=torch.int32, device=DEV)
    freqs = _angles(40, d)[:, None, None, :]
    t = _rand((T, h, d), dtype, 9)
    g = _rand((T, h, d), dtype, 10)

    def run():
        x = t.detach().requires_grad_(True)
        y = fr.fused_apply_rotary_pos_emb_thd(x, cu, freqs)
        (dx,) = torch.autograd.grad(y, x, g)
        return y.detach(), dx

    y, dx = run()
    xr = t.float().requires_grad_(True)
    yr = fr.rope_reference(xr, freqs.cos(), freqs.sin(), cu_seqlens=cu)
    (dr,) = torch.autograd.grad(yr, xr, g.float())
    _close(y, yr.detach(), dtype)
    _close(dx, dr, dtype)
    assert torch.equal(y[CU[-1]:], t[CU[-1]:]) and torch.equal(dx[CU[-1]:], g[CU[-1]:])
    # per-sequence application of the sbhd form gives the same bits
    for a, b in zip(CU[:-1], CU[1:]):
        if b > a:
            assert torch.equal(y[a:b], fr.fused_apply_rotary_pos_emb(t[a:b].unsqueeze(1), freqs[:b - a]).squeeze(1))
    # no host read of cu_seqlens: a synchronising call raises in this mode
    try:
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
    except Exception:  # mode unavailable in this torch build
        return
    try:
        y2, dx2 = run()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_angles(dtype):
    """Positions near 131072: the tables must be built in fp32 and never pass through a 16-bit dtype
    (bf16 angles there are off by whole turns)."""
    fr = _fr()
    S, D = 37, 64

    class Owner(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(4, 4)
            self.rot = fr.RotaryEmbedding(D)

    m = Owner().to(DEV).to(dtype)
    freqs = m.rot(S, offset=131072 - S, device=DEV)
    assert freqs.dtype == torch.float32 and freqs.is_cuda and float(freqs.max()) > 131000
    t = _rand((S, 2, 3, D), dtype, 11).requires_grad_(True)
    y = fr.fused_apply_rotary_pos_emb(t, freqs)
    g = _rand((S, 2, 3, D), dtype, 12)
    (dx,) = torch.autograd.grad(y, t, g)
    # the angles are the fp32 products pos * inv_freq bit for bit (one correctly rounded multiply each;
    # inv_freq itself is computed on the host, where the module builds it)
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    pos = torch.arange(S, dtype=torch.float32) + (131072 - S)
    ang = torch.outer(pos, inv)
    ang = torch.cat([ang, ang], -1).to(DEV)
    assert torch.equal(freqs[:, 0, 0], ang)
    xr = t.detach().float().requires_grad_(True)
    yr = fr.rope_reference(xr, ang.cos(), ang.sin())
    (dr,) = torch.autograd.grad(yr, xr, g.float())
    _close(y.detach(), yr.detach(), dtype)
    _close(dx, dr, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_repeatable(dtype):
    fr = _fr()
    ang = _angles(130, 64)
    qkv = _rand((2, 130, 3, 3, 64), dtype, 13).requires_grad_(True)
    g = _rand((2, 130, 3, 3, 64), dtype, 14)
    outs = []
    for _ in range(2):
        y = fr.apply_rotary_qkv_packed(qkv, ang.cos(), ang.sin())
        outs.append((y.detach().clone(), torch.autograd.grad(y, qkv, g)[0].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# --------------------------------------------------------------------------------------------
# models under amp O2 bf16: one forward + backward + FusedAdam step
# --------------------------------------------------------------------------------------------
# The band is the one tests/test_gpt_fused_gpu.py uses for bf16 model paths that differ only in
# fusion points (rtol = atol = 2e-2 there); the two losses here differ by far less, since both
# rotations compute in fp32 and round once.
MODEL_RTOL = 2e-2


def _one_step(model, batch, monkeypatch, c_layers):
    from apex import amp
    from apex.amp._amp_state import _amp_state
    from apex.optimizers import FusedAdam

    fr = _fr()
    _amp_state.optimizers, _amp_state.loss_scalers = [], []
    opt = FusedAdam(model.parameters(), lr=1e-3)
    model, opt = amp.initialize(model, opt, opt_level="O2", cast_model_type=torch.bfloat16, verbosity=0)
    calls = []
    with monkeypatch.context() as mp:
        mp.setattr(fr, "apply_rotary_qkv_packed",
                   lambda qkv, cos, sin: (calls.append(1), fr.rope_reference_qkv_packed(qkv, cos, sin))[1])
        with torch.no_grad():
            ref = float(model(*batch).float())
    assert len(calls) == c_layers
    loss = model(*batch)
    with amp.scale_loss(loss, opt) as sl:
        sl.backward()
    opt.step()
    opt.zero_grad()
    loss = float(loss.detach().float())
    print("rope loss", loss, "reference-rope loss", ref)
    assert loss == loss and abs(loss) != float("inf")
    assert abs(loss - ref) <= MODEL_RTOL * abs(ref)
    _amp_state.optimizers, _amp_state.loss_scalers = [], []


def test_gpt_rope_amp_o2(monkeypatch):
    from apex.models import GPTConfig, GPTModel

    torch.manual_seed(0)
    c = GPTConfig.tiny()
    c.dropout = 0.0
    c.position_embedding_type = "rope"
    m = GPTModel(c).to(DEV)
    assert not any("wpe" in k for k in m.state_dict())
    ids = torch.randint(0, c.vocab_size, (2, 64), device=DEV)
    _one_step(m, (ids, ids), monkeypatch, c.n_layer)
    c_, s_ = m.rotary_pos_emb.cos_sin(64, device=DEV)
    assert c_.dtype == torch.float32 and s_.dtype == torch.float32


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_megatron_rope_amp_o2(monkeypatch):
    import torch.distributed as dist

    from apex.models.megatron_gpt import MegatronGPTConfig, build_stage
    from apex.transformer import parallel_state as ps

    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_port()}", rank=0, world_size=1)
    ps.initialize_model_parallel(1, 1)
    try:
        torch.manual_seed(0)
        c = MegatronGPTConfig.tiny()
        c.hidden_dropout = c.attention_dropout = 0.0
        c.position_embedding_type = "rope"
        m = build_stage(c).to(DEV)
        assert not any("position_embeddings" in k for k in m.state_dict())
        ids = torch.randint(0, c.vocab_size, (2, 64), device=DEV)
        _one_step(m, (ids, ids), monkeypatch, c.num_layers)
    finally:
        ps.destroy_model_parallel()
        if own:
            dist.destroy_process_group()
