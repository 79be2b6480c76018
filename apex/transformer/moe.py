"""Mixture-of-experts MLP for the Megatron-style layers: a top-k router over ``num_experts`` expert MLPs that
run as grouped GEMMs on expert-sorted tokens (apex.ops.grouped), with no host read of the routing, and the
Switch / Megatron load-balancing auxiliary loss.

Out of scope here: expert parallelism, tensor-parallel (sharded) experts, capacity limits and token dropping,
a router z-loss, sequence-level auxiliary losses, and fp8 / MX experts.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from ..ops import fused as fops
from ..ops.grouped import grouped_linear, moe_permute, moe_route, moe_unpermute

_ACTS = {"gelu": None, "swiglu": fops.ACT_SILU, "geglu": fops.ACT_GELU}

_aux_loss_scale = 1.0


def set_aux_loss_scale(scale):
    """The factor (a float or a 0-dim tensor, default 1) every ``MoEMLP`` multiplies the gradient of its
    auxiliary loss by: the loss scale of mixed precision, one over the number of micro-batches."""
    global _aux_loss_scale
    _aux_loss_scale = scale


class _AuxLossScaler(torch.autograd.Function):
    """Identity on ``out`` that carries ``aux`` into the graph: the backward passes ``dout`` through and hands
    the aux-loss scale to ``aux`` as its gradient, so the loss trains on whichever pipeline stage the layer is
    without the model adding it to its own loss."""

    @staticmethod
    def forward(ctx, out, aux):
        ctx.like = aux.detach()
        return out.view_as(out)

    @staticmethod
    def backward(ctx, dout):
        aux, scale = ctx.like, _aux_loss_scale
        if torch.is_tensor(scale):
            return dout, scale.to(device=aux.device, dtype=aux.dtype).reshape(aux.shape)
        return dout, torch.full_like(aux, float(scale))


class MoEMLP(nn.Module):
    """``out[t] = sum_k gate[t, k] * MLP_{e(t, k)}(x[t])`` over the ``topk`` experts with the largest router
    logits; the gate is a softmax over those ``topk`` logits in fp32. ``activation``: "gelu" (erf), or the gated
    "swiglu" / "geglu", whose first expert weight emits ``[gate | up]`` as the dense gated MLP's does. Experts
    have no bias. Returns ``(out, None)``, the (output, bias) pair of the parallel linears.

    Routing is one call of ``apex.ops.moe_route``: equal logits go to the lowest expert index, on the CPU and
    on the device alike (``torch.topk`` leaves that order unspecified on the device).

    ``aux_loss_coeff`` > 0 adds the load-balancing loss ``coeff * E / (T^2 topk) * sum_e tokens_per_expert[e] *
    sum_t softmax(logits)[t, e]``: after a forward ``aux_loss`` holds its detached value, and its gradient
    reaches the router through the layer's output (times :func:`set_aux_loss_scale`), so nothing has to be
    added to the model's loss.

    Parameters: ``router.weight [E, hidden]``, ``w1 [E, ffn_hidden (x 2 when gated), hidden]``, ``w2 [E, hidden,
    ffn_hidden]``. After a forward, ``router_probs`` is the gate ``[tokens, topk]`` (fp32, attached to the graph),
    ``expert_ids`` the chosen experts and ``tokens_per_expert`` their counts ``[E]`` (both int64). See the
    module docstring for what is out of scope.

    ``score_function="sigmoid"`` with ``num_groups`` / ``group_topk`` and ``scaling_factor`` selects the sigmoid,
    group-limited router of ``apex.ops.moe_route`` (the gate is then the normalised, scaled sigmoid score).
    ``expert_bias=True`` adds the aux-loss-free balancing of that router: the fp32 buffer ``expert_bias [E]``
    enters the selection only, every training forward adds its token counts to the buffer
    ``tokens_per_expert_acc [E]`` (no host read), and :meth:`update_expert_bias`, called once per optimizer step,
    moves the bias towards the under-loaded experts."""

    def __init__(self, hidden, ffn_hidden, num_experts, topk=2, activation="gelu", init_std=0.02, out_std=None,
                 params_dtype=torch.float32, aux_loss_coeff=0.0, score_function="softmax", num_groups=None,
                 group_topk=None, scaling_factor=1.0, expert_bias=False):
        super().__init__()
        if activation not in _ACTS:
            raise ValueError(f"activation must be 'gelu', 'swiglu' or 'geglu', got {activation!r}")
        if not 1 <= topk <= num_experts:
            raise ValueError(f"topk={topk} must be in [1, num_experts={num_experts}]")
        self.num_experts, self.topk, self.gated_act = num_experts, topk, _ACTS[activation]
        self.aux_loss_coeff = float(aux_loss_coeff)
        if score_function not in ("softmax", "sigmoid"):
            raise ValueError(f"score_function must be 'softmax' or 'sigmoid', got {score_function!r}")
        if score_function != "sigmoid" and (num_groups is not None or group_topk is not None or expert_bias
                                            or scaling_factor != 1.0):
            raise ValueError("num_groups, group_topk, scaling_factor and expert_bias need score_function='sigmoid'")
        self.route_options = dict(score_function=score_function)
        if score_function == "sigmoid":
            self.route_options.update(num_groups=num_groups, group_topk=group_topk, scaling_factor=scaling_factor)
        if expert_bias:
            self.register_buffer("expert_bias", torch.zeros(num_experts, dtype=torch.float32))
            self.register_buffer("tokens_per_expert_acc", torch.zeros(num_experts, dtype=torch.float32))
        else:
            self.expert_bias = None
        self.router = nn.Linear(hidden, num_experts, bias=False, dtype=params_dtype)
        f1 = ffn_hidden if self.gated_act is None else 2 * ffn_hidden
        self.w1 = nn.Parameter(torch.empty(num_experts, f1, hidden, dtype=params_dtype))
        self.w2 = nn.Parameter(torch.empty(num_experts, hidden, ffn_hidden, dtype=params_dtype))
        nn.init.normal_(self.router.weight, 0.0, init_std)
        nn.init.normal_(self.w1, 0.0, init_std)
        nn.init.normal_(self.w2, 0.0, init_std if out_std is None else out_std)
        self.router_probs = self.expert_ids = self.tokens_per_expert = self.aux_loss = None

    def _act(self, h):
        if self.gated_act is not None:
            return fops.gated_act(h, None, self.gated_act)
        if fops._native(h) and h.shape[-1] % 8 == 0 and h.dtype in (torch.float32, torch.float16, torch.bfloat16):
            return fops._BiasAct.apply(h, None, fops.ACT_GELU)
        return F.gelu(h)

    def forward(self, x):
        x2 = x.reshape(-1, x.shape[-1])
        bias = {} if self.expert_bias is None else dict(expert_bias=self.expert_bias.float())
        r = moe_route(self.router(x2), self.topk, aux_loss=self.aux_loss_coeff != 0.0, **self.route_options, **bias)
        self.router_probs, self.expert_ids = r.probs, r.expert_ids.long()
        self.tokens_per_expert = r.tokens_per_expert.long()
        if self.expert_bias is not None and self.training:
            with torch.no_grad():
                self.tokens_per_expert_acc += r.tokens_per_expert
        xp, offsets, dest = moe_permute(x2, r.expert_ids, self.num_experts, routing=r)
        h = self._act(grouped_linear(xp, self.w1, offsets))   # zero rows stay zero through all three activations
        out = moe_unpermute(grouped_linear(h, self.w2, offsets), dest, r.probs, routing=r)
        self.aux_loss = None
        if r.aux_loss is not None:
            aux = self.aux_loss_coeff * r.aux_loss
            self.aux_loss = aux.detach()
            out = _AuxLossScaler.apply(out, aux)
        return out.view(x.shape), None

    @torch.no_grad()
    def update_expert_bias(self, rate):
        """``expert_bias += rate * sign(mean(acc) - acc)`` over the token counts accumulated since the last call,
        then the accumulator is zeroed: experts that got fewer tokens than the average become more likely."""
        if self.expert_bias is None:
            raise RuntimeError("update_expert_bias needs MoEMLP(..., expert_bias=True)")
        acc = self.tokens_per_expert_acc
        self.expert_bias += rate * torch.sign(acc.mean() - acc)
        acc.zero_()

    def extra_repr(self):
        return f"experts={self.num_experts}, topk={self.topk}, w1={tuple(self.w1.shape)}, w2={tuple(self.w2.shape)}"
