"""A tiny Llama-style GPT (rotary positions, grouped-query attention, SwiGLU MLP) on the GPU: one bf16 step
against the same weights in fp32 on the CPU, with the LayerNorms fused into the residual updates and
without, and the same step under apex.fp8.fp8_autocast.

The gated MLP path is fused_dense -> gated_act -> fused_dense. It never consumes a codes-only fp8
tensor: only apex.ops.blocks' whole-sublayer Functions ask a producer to skip its 16-bit output
(Fp8State.codes_only_ok); fused_dense goes through gemm.linear / gemm.dgrad, which make no such
request, and the gated path does not use fblocks.mlp."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _config():
    from apex.models.gpt import GPTConfig

    # ffn 344: F % 8 == 0 (the kernels' path) and no multiple of the 256-thread block's 2048 columns
    return GPTConfig(vocab_size=1000, n_positions=128, n_embd=128, n_layer=2, n_head=4, n_kv_head=2, dropout=0.0,
                     position_embedding_type="rope", activation="swiglu", ffn_hidden_size=344)


def _models():
    from apex.models.gpt import GPTModel

    torch.manual_seed(0)
    ref = GPTModel(_config())
    with torch.no_grad():   # zero-initialised biases would hide a misplaced one
        for p in ref.parameters():
            if p.ndim == 1:
                p.add_(torch.randn(p.shape) * 0.05)
    # the GPU model starts from the bf16-rounded weights; the fp32 reference takes the same values
    dev = copy.deepcopy(ref).cuda().to(torch.bfloat16)
    with torch.no_grad():
        for p, q in zip(ref.parameters(), dev.parameters()):
            p.copy_(q.float().cpu())
    ids = torch.randint(0, 1000, (2, 64), generator=torch.Generator().manual_seed(1))
    return ref, dev, ids


@pytest.mark.parametrize("fused_ln", [True, False])
def test_llama_style_step_bf16_vs_fp32_cpu(fused_ln, monkeypatch):
    from apex.models import gpt

    monkeypatch.setattr(gpt, "_FUSED_LN", fused_ln)
    ref, dev, ids = _models()
    assert dev.blocks[0].c_fc.weight.shape == (688, 128)
    want = ref(ids, ids)
    want.backward()
    got = dev(ids.cuda(), ids.cuda())
    got.backward()
    print(f"loss bf16 GPU {float(got.detach()):.5f}, fp32 CPU {float(want.detach()):.5f}")
    torch.testing.assert_close(got.float().cpu(), want.detach(), rtol=2e-2, atol=2e-2)
    errs = {}
    for (n, p), q in zip(ref.named_parameters(), dev.parameters()):
        assert q.grad is not None and bool(torch.isfinite(q.grad.float()).all()), n
        errs[n] = float((q.grad.float().cpu() - p.grad).norm() / p.grad.norm().clamp_min(1e-12))
    print({n: round(e, 5) for n, e in errs.items()})
    assert max(errs.values()) < 2e-2, errs


def test_llama_style_step_fp8_tracks_bf16():
    """The gated step under fp8_autocast: finite, and the loss within the band tests/test_fp8_gpu.py uses
    for "fp8 loss tracks bf16" (5 % + 0.05)."""
    from apex import fp8

    fp8.disable()
    _, dev, ids = _models()
    ids = ids.cuda()
    try:
        ref = dev(ids, ids)
        ref.backward()
        dev.zero_grad(set_to_none=True)
        with fp8.fp8_autocast():
            got = dev(ids, ids)
            got.backward()
        n_slots = fp8.state().n
    finally:
        fp8.disable()
    got, ref = got.detach(), ref.detach()
    print(f"loss fp8 {float(got):.5f}, bf16 {float(ref):.5f}, fp8 slots {n_slots}")
    assert n_slots > 0   # some GEMM did run in fp8
    assert bool(torch.isfinite(got))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad.float()).all()) for p in dev.parameters())
    assert abs(float(got) - float(ref)) <= 0.05 * float(ref) + 0.05
