"""MoEMLP (apex.transformer.moe) on the CPU tier — the PyTorch path of apex.ops.grouped — against a float64 dense
formulation that runs every expert on every token and keeps its output with a 0/1 mask; and the
MegatronGPTConfig.num_moe_experts option."""
import pytest
import torch
import torch.nn.functional as F

from apex.models.megatron_gpt import MegatronGPT, MegatronGPTConfig
from apex.transformer import parallel_state as ps
from apex.transformer.moe import MoEMLP
from test_transformer import _spawn

T, H, FFN, E = 40, 16, 24, 4


def dense_moe64(x, wr, w1, w2, topk, activation):
    logits = (x.float() @ wr.float().t()).double()   # the layer's router runs in the parameter dtype (fp32 here)
    top, ids = torch.topk(logits, topk, -1)
    probs = torch.softmax(top, -1)
    out = torch.zeros_like(x)
    for e in range(E):
        h = x @ w1[e].t()
        if activation == "gelu":
            a = F.gelu(h)
        else:
            g, u = h.chunk(2, -1)
            a = (F.silu(g) if activation == "swiglu" else F.gelu(g)) * u
        gate = (probs * (ids == e)).sum(-1, keepdim=True)   # 0/1 mask times the gate
        out = out + gate * (a @ w2[e].t())
    return out


@pytest.mark.parametrize("topk", [1, 2])
@pytest.mark.parametrize("activation", ["gelu", "swiglu", "geglu"])
def test_moe_mlp_matches_dense_float64(activation, topk):
    torch.manual_seed(3)
    m = MoEMLP(H, FFN, E, topk, activation, init_std=0.3)
    x = torch.randn(T, H, requires_grad=True)
    dout = torch.randn(T, H)
    out, bias = m(x)
    assert bias is None and out.shape == x.shape
    assert int(m.tokens_per_expert.sum()) == T * topk and m.router_probs.shape == (T, topk)
    got = torch.autograd.grad(out, [x, m.router.weight, m.w1, m.w2], dout)
    p64 = [t.detach().double().requires_grad_() for t in (x, m.router.weight, m.w1, m.w2)]
    ref = dense_moe64(*p64, topk, activation)
    ref_g = torch.autograd.grad(ref, p64, dout.double())
    # fp32 against float64 at |values| of order 1 and contractions of at most 48 terms: 1e-4 is a hundredfold
    # of the accumulated fp32 rounding and far below any wrong row, gate or mask
    for name, g, r in zip(["out", "dx", "drouter", "dw1", "dw2"], (out,) + got, (ref,) + ref_g):
        assert torch.allclose(g.double(), r, rtol=1e-4, atol=1e-4), (name, float((g.double() - r).abs().max()))


def _megatron_experts(rank, world):
    ps.initialize_model_parallel(1, 1)

    def cfg(**kw):
        return MegatronGPTConfig(vocab_size=64, hidden_size=32, num_layers=2, num_attention_heads=2,
                                 max_position_embeddings=16, hidden_dropout=0.0, attention_dropout=0.0, **kw)

    torch.manual_seed(0)
    model = MegatronGPT(cfg(num_moe_experts=4))
    ids = torch.randint(0, 64, (2, 16))
    loss = model(ids, labels=ids)
    loss.backward()
    assert torch.isfinite(loss)
    mlp = model.layers[0].mlp
    assert mlp.topk == 2 and mlp.w1.shape == (4, 128, 32) and mlp.w2.shape == (4, 32, 128)
    for p in (mlp.router.weight, mlp.w1, mlp.w2):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0

    # num_moe_experts=None: the parameter names of the parent commit, as a literal list
    layer = ["input_layernorm.weight", "input_layernorm.bias", "query_key_value.weight", "query_key_value.bias",
             "dense.weight", "dense.bias", "post_attention_layernorm.weight", "post_attention_layernorm.bias",
             "dense_h_to_4h.weight", "dense_h_to_4h.bias", "dense_4h_to_h.weight", "dense_4h_to_h.bias"]
    assert cfg().num_moe_experts is None
    assert list(MegatronGPT(cfg()).state_dict().keys()) == (
        ["word_embeddings.weight", "position_embeddings.weight"] + [f"layers.{i}.{k}" for i in (0, 1) for k in layer]
        + ["final_layernorm.weight", "final_layernorm.bias"])

    # experts are not sharded: a tensor-parallel world size above 1 is refused
    real = ps.get_tensor_model_parallel_world_size
    ps.get_tensor_model_parallel_world_size = lambda: 2
    try:
        with pytest.raises(ValueError, match="tensor-parallel"):
            MegatronGPT(cfg(num_moe_experts=4))
    finally:
        ps.get_tensor_model_parallel_world_size = real


def test_megatron_num_moe_experts():
    _spawn(_megatron_experts, 1)
