"""Mixture-of-experts MLP for the Megatron-style layers: a top-k router over ``num_experts`` expert MLPs that
run as grouped GEMMs on expert-sorted tokens (apex.ops.grouped), with no host read of the routing.

Out of scope here: expert parallelism, tensor-parallel (sharded) experts, a load-balancing auxiliary loss (the
layer keeps ``router_probs`` and ``tokens_per_expert`` of its last forward so one can be added), capacity
limits and token dropping, and fp8 / MX experts.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from ..ops import fused as fops
from ..ops.grouped import grouped_linear, moe_permute, moe_unpermute

_ACTS = {"gelu": None, "swiglu": fops.ACT_SILU, "geglu": fops.ACT_GELU}


class MoEMLP(nn.Module):
    """``out[t] = sum_k gate[t, k] * MLP_{e(t, k)}(x[t])`` over the ``topk`` experts with the largest router
    logits; the gate is a softmax over those ``topk`` logits in fp32. ``activation``: "gelu" (erf), or the gated
    "swiglu" / "geglu", whose first expert weight emits ``[gate | up]`` as the dense gated MLP's does. Experts
    have no bias. Returns ``(out, None)``, the (output, bias) pair of the parallel linears.

    Parameters: ``router.weight [E, hidden]``, ``w1 [E, ffn_hidden (x 2 when gated), hidden]``, ``w2 [E, hidden,
    ffn_hidden]``. After a forward, ``router_probs`` is the gate ``[tokens, topk]`` (fp32, attached to the graph),
    ``expert_ids`` the chosen experts and ``tokens_per_expert`` their counts ``[E]``. See the module docstring
    for what is out of scope."""

    def __init__(self, hidden, ffn_hidden, num_experts, topk=2, activation="gelu", init_std=0.02, out_std=None,
                 params_dtype=torch.float32):
        super().__init__()
        if activation not in _ACTS:
            raise ValueError(f"activation must be 'gelu', 'swiglu' or 'geglu', got {activation!r}")
        if not 1 <= topk <= num_experts:
            raise ValueError(f"topk={topk} must be in [1, num_experts={num_experts}]")
        self.num_experts, self.topk, self.gated_act = num_experts, topk, _ACTS[activation]
        self.router = nn.Linear(hidden, num_experts, bias=False, dtype=params_dtype)
        f1 = ffn_hidden if self.gated_act is None else 2 * ffn_hidden
        self.w1 = nn.Parameter(torch.empty(num_experts, f1, hidden, dtype=params_dtype))
        self.w2 = nn.Parameter(torch.empty(num_experts, hidden, ffn_hidden, dtype=params_dtype))
        nn.init.normal_(self.router.weight, 0.0, init_std)
        nn.init.normal_(self.w1, 0.0, init_std)
        nn.init.normal_(self.w2, 0.0, init_std if out_std is None else out_std)
        self.router_probs = self.expert_ids = self.tokens_per_expert = None

    def _act(self, h):
        if self.gated_act is not None:
            return fops.gated_act(h, None, self.gated_act)
        if fops._native(h) and h.shape[-1] % 8 == 0 and h.dtype in (torch.float32, torch.float16, torch.bfloat16):
            return fops._BiasAct.apply(h, None, fops.ACT_GELU)
        return F.gelu(h)

    def forward(self, x):
        x2 = x.reshape(-1, x.shape[-1])
        logits = self.router(x2).float()
        top, ids = torch.topk(logits, self.topk, dim=-1)
        probs = torch.softmax(top, dim=-1)
        self.router_probs, self.expert_ids = probs, ids
        self.tokens_per_expert = torch.zeros(self.num_experts, dtype=torch.long, device=ids.device).scatter_add_(
            0, ids.reshape(-1), torch.ones_like(ids.reshape(-1)))
        xp, offsets, dest = moe_permute(x2, ids, self.num_experts)
        h = self._act(grouped_linear(xp, self.w1, offsets))   # zero rows stay zero through all three activations
        out = moe_unpermute(grouped_linear(h, self.w2, offsets), dest, probs)
        return out.view(x.shape), None

    def extra_repr(self):
        return f"experts={self.num_experts}, topk={self.topk}, w1={tuple(self.w1.shape)}, w2={tuple(self.w2.shape)}"

