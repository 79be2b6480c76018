"""Megatron-style GPT over apex.transformer — BASELINE.json config 5 ("apex.transformer
Megatron-style GPT, TP=4 PP=2 over xGMI on 8x MI355X").

Each pipeline stage owns a contiguous range of decoder layers; layer internals are
tensor-parallel: QKV and fc1 are ColumnParallelLinear (heads / FFN columns split across the
TP group, no gather), out-proj and fc2 are RowParallelLinear (one RCCL all-reduce each),
attention runs the causal MFMA flash kernel on the rank-local heads. Stage 0 holds the
vocab-parallel token embedding, the last stage the vocab-parallel LM head (tied to the
embedding: its gradient is all-reduced over the embedding group) and computes
vocab_parallel_cross_entropy on sharded logits.
"""
from __future__ import annotations

import contextlib
import math
import os
from dataclasses import dataclass

import torch
import torch.distributed as dist
import torch.nn.functional as F
from torch import nn

from ..normalization import FusedLayerNorm
from ..ops import blocks as fblocks
from ..ops import fused as fops
from ..transformer import parallel_state as ps
from ..transformer import tensor_parallel as tp
from ..transformer.functional import fused_rope


# APEX_MEGATRON_FUSED_LN=0: per-layer forward (separate LayerNorms; A/B and fallback switch)
_FUSED_LN = os.environ.get("APEX_MEGATRON_FUSED_LN", "1") != "0"

# MegatronGPTConfig.activation -> the gated activation's code (None: the plain bias + GELU(erf) MLP)
_ACTIVATIONS = {"gelu": None, "swiglu": fops.ACT_SILU, "geglu": fops.ACT_GELU}


@dataclass
class MegatronGPTConfig:
    vocab_size: int = 50304
    hidden_size: int = 2048
    num_layers: int = 24
    num_attention_heads: int = 16
    ffn_hidden_size: int = None
    max_position_embeddings: int = 2048
    hidden_dropout: float = 0.1
    attention_dropout: float = 0.1
    layernorm_epsilon: float = 1e-5
    init_method_std: float = 0.02
    params_dtype: torch.dtype = torch.float32
    position_embedding_type: str = "learned"  # "learned" | "rope"
    rotary_percent: float = 1.0
    rotary_base: int = 10000
    num_query_groups: int | None = None  # grouped-query attention: key/value heads (None = num_attention_heads)
    activation: str = "gelu"  # "gelu" | "swiglu" | "geglu" (gated: dense_h_to_4h emits [gate | up], erf GELU)

    def __post_init__(self):
        if self.activation not in _ACTIVATIONS:
            raise ValueError(f"activation must be 'gelu', 'swiglu' or 'geglu', got {self.activation!r}")
        g = self.num_query_groups
        if g is not None and (g < 1 or self.num_attention_heads % g):
            raise ValueError(f"num_attention_heads={self.num_attention_heads} must be a multiple of "
                             f"num_query_groups={g}")
        if self.ffn_hidden_size is None:
            self.ffn_hidden_size = 4 * self.hidden_size
        if self.position_embedding_type not in ("learned", "rope"):
            raise ValueError(f"position_embedding_type must be 'learned' or 'rope', got "
                             f"{self.position_embedding_type!r}")

    @staticmethod
    def tiny():
        return MegatronGPTConfig(vocab_size=512, hidden_size=128, num_layers=4, num_attention_heads=4,
                                 max_position_embeddings=64)


def _init(std):
    return lambda w: nn.init.normal_(w, 0.0, std)


def _tp_rng():
    """Dropout on tensor-parallel shards (attention probabilities) draws from the tracked
    'model-parallel-rng' state: a different mask on every TP rank, the same on DP replicas."""
    tr = tp.get_cuda_rng_tracker()
    return tr.fork() if "model-parallel-rng" in tr.get_states() else contextlib.nullcontext()


class ParallelTransformerLayer(nn.Module):
    # Gated MLP (activation "swiglu" / "geglu"): dense_h_to_4h is [2 * ffn_hidden_size, hidden] and every
    # rank's shard of it (and of its bias) is laid out rank-locally as its ffn/tp gate rows, then its
    # ffn/tp up rows, the rule the query_key_value shard follows for Q / K / V. gated_act on the local
    # [.., 2 ffn/tp] output therefore pairs each gate column with its own up column and needs nothing
    # from the TP group; the TP = 1 weight is [cat_r(gate_r); cat_r(up_r)].
    def __init__(self, c: MegatronGPTConfig, layer_number):
        super().__init__()
        tpws = ps.get_tensor_model_parallel_world_size()
        self.heads_local = tp.divide(c.num_attention_heads, tpws)
        self.d = c.hidden_size // c.num_attention_heads
        out_std = c.init_method_std / math.sqrt(2.0 * c.num_layers)
        self.input_layernorm = FusedLayerNorm(c.hidden_size, eps=c.layernorm_epsilon)
        # grouped-query attention: every rank's shard of query_key_value is laid out rank-locally as its
        # query heads, then its key heads, then its value heads ([3, heads_local, d] when groups == heads)
        groups = c.num_attention_heads if c.num_query_groups is None else c.num_query_groups
        if groups % tpws:
            raise ValueError(f"num_query_groups={groups} must be a multiple of the tensor-parallel world size {tpws}")
        self.groups_local = groups // tpws
        qkv_out = 3 * c.hidden_size if groups == c.num_attention_heads else (c.num_attention_heads + 2 * groups) * self.d
        self.query_key_value = tp.ColumnParallelLinear(c.hidden_size, qkv_out, gather_output=False,
                                                       init_method=_init(c.init_method_std),
                                                       params_dtype=c.params_dtype)
        self.dense = tp.RowParallelLinear(c.hidden_size, c.hidden_size, input_is_parallel=True,
                                          init_method=_init(out_std), skip_bias_add=True, params_dtype=c.params_dtype)
        self.post_attention_layernorm = FusedLayerNorm(c.hidden_size, eps=c.layernorm_epsilon)
        self.gated_act = _ACTIVATIONS[c.activation]
        if self.gated_act is not None and c.ffn_hidden_size % tpws:
            raise ValueError(f"ffn_hidden_size={c.ffn_hidden_size} must be a multiple of the tensor-parallel "
                             f"world size {tpws}")
        f1_out = c.ffn_hidden_size if self.gated_act is None else 2 * c.ffn_hidden_size
        self.dense_h_to_4h = tp.ColumnParallelLinear(c.hidden_size, f1_out, gather_output=False,
                                                     init_method=_init(c.init_method_std), skip_bias_add=True,
                                                     params_dtype=c.params_dtype)
        self.dense_4h_to_h = tp.RowParallelLinear(c.ffn_hidden_size, c.hidden_size, input_is_parallel=True,
                                                  init_method=_init(out_std), skip_bias_add=True,
                                                  params_dtype=c.params_dtype)
        self.p_hidden, self.p_attn = c.hidden_dropout, c.attention_dropout

    def _rotate(self, qkv, rope):
        # rope = (cos, sin) [S, d2] fp32 or None (learned positions). RoPE is per head, so the
        # rank-local heads need nothing from the TP group. No fp8 interaction: the fp8 codes-only
        # paths live in apex.ops.blocks' whole-sublayer Functions, which this attention sublayer does
        # not use (QKV GEMM, this rotation and the flash kernel are separate bf16 / fp16 ops).
        return qkv if rope is None else fused_rope.apply_rotary_qkv_packed(qkv, rope[0], rope[1])

    def _attn(self, qkv, rope, pa):
        B, S = qkv.shape[:2]
        h, hk = self.heads_local, self.groups_local
        if hk != h:
            qkv = qkv.view(B, S, h + 2 * hk, self.d)
            if rope is not None:
                qkv = fused_rope.apply_rotary_qkv_grouped(qkv, rope[0], rope[1], h, hk)
            with _tp_rng():
                return fops.attention_qkv_grouped(qkv, h, hk, None, pa, causal=True)
        qkv = self._rotate(qkv.view(B, S, 3, self.heads_local, self.d), rope)
        with _tp_rng():
            return fops.attention_qkv_packed(qkv, None, pa, causal=True)

    def _gated_mlp(self, xn):
        # through the two parallel linears (their TP / sequence-parallel mappings), the rank-local
        # [gate | up] shard between them; not fblocks.mlp. Under apex.fp8.fp8_autocast the linears'
        # outputs are never codes-only: only apex.ops.blocks' whole-sublayer Functions request one.
        h, b1 = self.dense_h_to_4h(xn)
        return self.dense_4h_to_h(fops.gated_act(h, b1, self.gated_act))

    def forward(self, x, rope=None):
        B, S, _ = x.shape
        ph = self.p_hidden if self.training else 0.0
        pa = self.p_attn if self.training else 0.0
        qkv, _ = self.query_key_value(self.input_layernorm(x))
        ctx = self._attn(qkv, rope, pa)
        out, bias = self.dense(ctx.reshape(B, S, -1))
        x = fops.bias_dropout_add(out, bias, x, ph)
        xn = self.post_attention_layernorm(x)
        f1, f2 = self.dense_h_to_4h, self.dense_4h_to_h
        if self.gated_act is not None:
            out, bias = self._gated_mlp(xn)
            return fops.bias_dropout_add(out, bias, x, ph)
        if not (f1.sequence_parallel_enabled or f2.sequence_parallel_enabled) and f1.bias is not None:
            # whole MLP shard as one Function (GEMM+bias+GELU epilogue, dGELU epilogue in backward)
            # between the same TP mappings the two parallel linears apply
            t = fblocks.mlp(tp.copy_to_tensor_model_parallel_region(xn), f1.weight, f1.bias, f2.weight)
            if t is not None:
                return fops.bias_dropout_add(tp.reduce_from_tensor_model_parallel_region(t), f2.bias, x, ph)
        h, b1 = f1(xn)
        h = fops.bias_gelu(h, b1) if b1 is not None else F.gelu(h)
        out, bias = f2(h)
        return fops.bias_dropout_add(out, bias, x, ph)

    def forward_fused(self, x, xn, nxt, rope=None):
        """forward() with each residual update fused with the LayerNorm after it (one bdaln kernel
        each way, fops.bias_dropout_add_ln): takes x and xn = input_layernorm(x), returns
        (x', nxt(x')) with nxt the next layer's input_layernorm / the final LayerNorm, or (x', None)
        at a pipeline-stage boundary (the next stage normalises its own input)."""
        B, S, _ = x.shape
        ph = self.p_hidden if self.training else 0.0
        pa = self.p_attn if self.training else 0.0
        qkv, _ = self.query_key_value(xn)
        ctx = self._attn(qkv, rope, pa)
        out, bias = self.dense(ctx.reshape(B, S, -1))
        ln2 = self.post_attention_layernorm
        x, xn = fops.bias_dropout_add_ln(out, bias, x, ln2.weight, ln2.bias, ph, ln2.eps)
        f1, f2 = self.dense_h_to_4h, self.dense_4h_to_h
        t = bias2 = None
        if self.gated_act is not None:
            t, bias2 = self._gated_mlp(xn)
        elif not (f1.sequence_parallel_enabled or f2.sequence_parallel_enabled) and f1.bias is not None:
            t = fblocks.mlp(tp.copy_to_tensor_model_parallel_region(xn), f1.weight, f1.bias, f2.weight)
            if t is not None:
                t, bias2 = tp.reduce_from_tensor_model_parallel_region(t), f2.bias
        if t is None:
            h, b1 = f1(xn)
            h = fops.bias_gelu(h, b1) if b1 is not None else F.gelu(h)
            t, bias2 = f2(h)
        if nxt is None:
            return fops.bias_dropout_add(t, bias2, x, ph), None
        return fops.bias_dropout_add_ln(t, bias2, x, nxt.weight, nxt.bias, ph, nxt.eps)


class MegatronGPT(nn.Module):
    """One pipeline stage of the GPT (pre_process: embeddings, post_process: head + loss)."""

    def __init__(self, c: MegatronGPTConfig, pre_process=True, post_process=True, layer_offset=0,
                 num_local_layers=None):
        super().__init__()
        self.config = c
        self.pre_process, self.post_process = pre_process, post_process
        n = c.num_layers if num_local_layers is None else num_local_layers
        self.rope = c.position_embedding_type == "rope"
        if self.rope:
            # every pipeline stage builds its own tables from S (no parameters, nothing in state_dict)
            self.rotary_pos_emb = fused_rope.RotaryEmbedding(c.hidden_size // c.num_attention_heads,
                                                             c.rotary_percent, c.rotary_base)
        if pre_process:
            self.word_embeddings = tp.VocabParallelEmbedding(c.vocab_size, c.hidden_size,
                                                             init_method=_init(c.init_method_std),
                                                             params_dtype=c.params_dtype)
            if not self.rope:
                self.position_embeddings = nn.Embedding(c.max_position_embeddings, c.hidden_size)
                nn.init.normal_(self.position_embeddings.weight, 0.0, c.init_method_std)
        self.layers = nn.ModuleList([ParallelTransformerLayer(c, layer_offset + i + 1) for i in range(n)])
        if post_process:
            self.final_layernorm = FusedLayerNorm(c.hidden_size, eps=c.layernorm_epsilon)
            if not pre_process:
                # LM head copy of the (tied) embedding on the last stage; grads synced over the
                # embedding group (first + last stage)
                self.word_embeddings = tp.VocabParallelEmbedding(c.vocab_size, c.hidden_size,
                                                                 init_method=_init(c.init_method_std),
                                                                 params_dtype=c.params_dtype)
        self.input_tensor = None

    def set_input_tensor(self, input_tensor):
        self.input_tensor = input_tensor

    def forward(self, input_ids, labels=None):
        if self.pre_process:
            S = input_ids.shape[1]
            if self.rope:
                x = self.word_embeddings(input_ids)
            else:
                if S > self.config.max_position_embeddings:  # host-side check (a bad gather faults the GPU)
                    raise ValueError(f"sequence length {S} exceeds max_position_embeddings="
                                     f"{self.config.max_position_embeddings}")
                pos = torch.arange(S, device=input_ids.device)
                x = self.word_embeddings(input_ids) + self.position_embeddings(pos)[None]
            x = F.dropout(x, self.config.hidden_dropout, self.training)
        else:
            x = self.input_tensor
        rope = self.rotary_pos_emb.cos_sin(x.shape[1], device=x.device) if self.rope else None
        if _FUSED_LN and len(self.layers):
            # residual stream with each LayerNorm fused into the residual update before it
            xn = self.layers[0].input_layernorm(x)
            for i, layer in enumerate(self.layers):
                if i + 1 < len(self.layers):
                    nxt = self.layers[i + 1].input_layernorm
                else:
                    nxt = self.final_layernorm if self.post_process else None
                x, xn = layer.forward_fused(x, xn, nxt, rope)
            if self.post_process:
                return self._head(xn, labels)
            return x
        for layer in self.layers:
            x = layer(x, rope)
        if not self.post_process:
            return x
        return self._head(self.final_layernorm(x), labels)

    def _head(self, x, labels):
        logits = fops.fused_dense(tp.copy_to_tensor_model_parallel_region(x), self.word_embeddings.weight, None)
        if labels is None:
            return logits
        shifted = torch.cat([labels[:, 1:], labels[:, -1:]], 1)
        loss = tp.vocab_parallel_cross_entropy(logits, shifted)  # fp32 statistics inside
        return loss[:, :-1].mean()


def build_stage(c: MegatronGPTConfig):
    """The GPT stage for this rank's pipeline position (layers split evenly)."""
    pp = ps.get_pipeline_model_parallel_world_size()
    r = ps.get_pipeline_model_parallel_rank()
    per = tp.divide(c.num_layers, pp)
    return MegatronGPT(c, pre_process=(r == 0), post_process=(r == pp - 1), layer_offset=r * per,
                       num_local_layers=per)


def sync_embedding_grads(model):
    """All-reduce the tied word-embedding grad between the first and last pipeline stage."""
    if ps.get_pipeline_model_parallel_world_size() == 1 or not ps.is_rank_in_embedding_group(True):
        return
    if not (model.pre_process or model.post_process):
        return
    w = model.word_embeddings.weight
    g = getattr(w, "main_grad", None)  # apex DDP fp32_main_grad mode: the fp32 accumulator
    if g is None:
        g = w.grad
        if g is None:
            g = torch.zeros_like(w)
            w.grad = g
    dist.all_reduce(g, group=ps.get_embedding_group())


def sync_initial_embeddings(model):
    """Make the last stage's LM-head copy equal to stage 0's embedding (call once)."""
    if ps.get_pipeline_model_parallel_world_size() == 1 or not ps.is_rank_in_embedding_group(True):
        return
    if not (model.pre_process or model.post_process):
        return
    w = model.word_embeddings.weight
    with torch.no_grad():
        if not model.pre_process:
            w.zero_()
        dist.all_reduce(w.data, group=ps.get_embedding_group())
