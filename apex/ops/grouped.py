"""Grouped linear layers over expert-sorted rows, and the token permutation around them (mixture of experts).

The segment layout every function here shares: expert-sorted activations are a 2-D tensor ``x [R, K]`` plus
``offsets``, an int32 device tensor ``[E + 1]`` with ``offsets[0] == 0``, non-decreasing entries that are all
multiples of 64, and ``offsets[E] <= R``. Expert ``e`` owns rows ``[offsets[e], offsets[e + 1])`` (possibly
none); the rows that pad a segment up to its multiple of 64 hold zeros; rows from ``offsets[E]`` on are an
unused tail that every op here writes as zeros. ``R`` is a static upper bound, so no shape depends on the
routing, and ``offsets`` is never read on the host: there is no sync, and everything here can be captured in
a ``torch.cuda.graph``.

  grouped_linear(x, weight, offsets)         y[seg_e] = x[seg_e] @ weight[e].T,  weight [E, N, K], no bias
  moe_route(logits, topk, aux_loss)          router logits [T, E] -> gate, expert ids, row maps, aux loss
  moe_permute(x, expert_ids, num_experts)    tokens [T, H] -> (xp [R, H], offsets, dest [T, topk])
  moe_unpermute(yp, dest, probs)             out[t] = sum_k probs[t, k] * yp[dest[t, k]]

Device tensors in bf16 / fp16 run on the HIP kernels of csrc/gemm_grouped.hip (one launch per GEMM: forward,
input gradient, weight gradient), csrc/moe.hip and csrc/moe_route.hip (routing and row maps). CPU tensors, ``APEX_FORCE_REFERENCE=1`` and the shapes
``grouped_gemm_supported`` declines take the PyTorch formulation below, which keeps the same contract (zero
pads, zero tail, no host read of ``offsets``).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from .. import _ext
from .fused import main_grad_placeholder

_HALF = (torch.bfloat16, torch.float16)


def grouped_gemm_supported(R, K, N, E):
    """Can the grouped MFMA kernels run ``[R, K] x [E, N, K]``? ``K % 64 == 0``, ``N % 8 == 0``, ``E >= 1``,
    ``R % 64 == 0`` and the kernels' size limits. Needs the built extension."""
    return bool(_ext.require().gemm_grouped_supported(int(R), int(K), int(N), int(E)))


def _native_gemm(a, R, K, N, E):
    return (_ext.use_native(a) and a.dtype in _HALF and a.is_contiguous() and a.data_ptr() % 16 == 0
            and grouped_gemm_supported(R, K, N, E))


def _row_expert(offsets, R):
    """Expert of every row ([R] int64; E for the tail), from the device-side table."""
    rows = torch.arange(R, device=offsets.device, dtype=offsets.dtype)
    return torch.bucketize(rows, offsets[1:].contiguous(), right=True)


def _nt_reference(x, w, offsets):
    """y[seg_e] = x[seg_e] @ w[e].T with a 0/1 row mask per expert (no host read of offsets); fp32 math for
    16-bit operands, rounded once; tail rows come out zero."""
    ct = torch.float32 if x.dtype in _HALF else x.dtype
    eid = _row_expert(offsets, x.shape[0])
    xf = x.to(ct)
    y = torch.zeros(x.shape[0], w.shape[1], dtype=ct, device=x.device)
    for e in range(w.shape[0]):
        y = y + (xf * (eid == e).to(ct)[:, None]) @ w[e].to(ct).t()
    return y.to(x.dtype)


def _tt_reference(dy, x, offsets, E):
    """dw[e] = dy[seg_e].T @ x[seg_e] in fp32 (float64 operands: float64), [E, N, K]."""
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    eid = _row_expert(offsets, x.shape[0])
    xf, dyf = x.to(ct), dy.to(ct)
    return torch.stack([(dyf * (eid == e).to(ct)[:, None]).t() @ xf for e in range(E)])


def _grouped_nt(x, w, offsets):
    if _native_gemm(x, x.shape[0], x.shape[1], w.shape[1], w.shape[0]) and w.is_contiguous() and w.data_ptr() % 16 == 0:
        return _ext.require().gemm_grouped_nt(x, w, offsets)
    return _nt_reference(x, w, offsets)


class _GroupedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, offsets):
        xc = x.contiguous()
        ctx.save_for_backward(xc, weight, offsets)
        ctx.param = weight
        return _grouped_nt(xc, weight.contiguous(), offsets)

    @staticmethod
    def backward(ctx, dy):
        x, w, offsets = ctx.saved_tensors
        E, N, K = w.shape
        dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            # the dense layers' convention: a per-step transposed copy of the weight, then the NT kernel
            dx = _grouped_nt(dy, w.transpose(1, 2).contiguous(), offsets)
        if ctx.needs_input_grad[1]:
            native = _native_gemm(x, x.shape[0], K, N, E) and dy.data_ptr() % 16 == 0
            mg = getattr(ctx.param, "main_grad", None)
            if mg is not None:
                if native and mg.dtype == torch.float32 and mg.is_contiguous() and mg.data_ptr() % 16 == 0 \
                        and mg.numel() == w.numel():
                    _ext.require().gemm_grouped_tt(dy, x, offsets, acc=mg)
                else:
                    mg.add_(_tt_reference(dy, x, offsets, E).view_as(mg).to(mg.dtype))
                dw = main_grad_placeholder(ctx.param)
            elif native:
                dw = _ext.require().gemm_grouped_tt(dy, x, offsets)
            else:
                dw = _tt_reference(dy, x, offsets, E).to(w.dtype)
        return dx, dw, None


def grouped_linear(x, weight, offsets):
    """``y[offsets[e]:offsets[e+1]] = x[offsets[e]:offsets[e+1]] @ weight[e].T`` for ``x [R, K]``, ``weight
    [E, N, K]`` and the int32 device table ``offsets [E + 1]`` of the module docstring; returns ``[R, N]`` with
    zero tail rows. No bias. Differentiable in ``x`` and ``weight``: the input gradient runs the same grouped
    kernel against a transposed copy of the weight, the weight gradient the grouped transposed-read kernel,
    accumulated in fp32 into ``weight.main_grad`` (a placeholder gradient is returned) when the parameter
    carries one. An expert without rows gets a zero gradient and leaves its ``main_grad`` slab untouched."""
    if x.dim() != 2 or weight.dim() != 3 or weight.shape[2] != x.shape[1]:
        raise ValueError(f"grouped_linear: x [R, K] and weight [E, N, K], got {tuple(x.shape)} and {tuple(weight.shape)}")
    if offsets.dtype != torch.int32 or offsets.shape != (weight.shape[0] + 1,) or offsets.device != x.device:
        raise ValueError("grouped_linear: offsets must be an int32 [E + 1] tensor on x's device")
    return _GroupedLinear.apply(x, weight, offsets)


# ---------------------------------------------------------------------------
# token permutation
def _native_rows(src, rows):
    return _ext.use_native(src) and src.is_contiguous() and src.data_ptr() % 16 == 0 and \
        _ext.require().moe_rows_supported(src, rows)


def _gather(src, row_of, scale=None):
    """out[r] = scale[r] * src[row_of[r]], zeros where row_of[r] < 0."""
    src = src.contiguous()
    if _native_rows(src, row_of.numel()):
        return _ext.require().moe_gather(src, row_of, scale)
    out = src[row_of.clamp(min=0).long()]
    if scale is not None:
        out = (out.float() * scale[:, None]).to(src.dtype)
    return torch.where((row_of >= 0)[:, None], out, torch.zeros_like(out))


def _combine(src, dest, w=None, g=None, want_out=True):
    """(sum_k w[t, k] * src[dest[t, k]] or None, <g[t], src[dest[t, k]]> in fp32 or None)."""
    src = src.contiguous()
    if g is not None:
        g = g.contiguous()
    if _native_rows(src, dest.shape[0]) and dest.shape[1] <= 8 and (g is None or g.data_ptr() % 16 == 0):
        return tuple(_ext.require().moe_combine(src, dest, w, g, want_out))
    ct = torch.float32 if src.dtype in _HALF else src.dtype
    rows = src[dest.long()].to(ct)                       # [T, topk, H]
    out = dw = None
    if want_out:
        out = (rows if w is None else rows * w.to(ct)[..., None]).sum(1).to(src.dtype)
    if g is not None:
        dw = (rows * g.to(ct)[:, None, :]).sum(-1).float()
    return out, dw


def _routing_maps(expert_ids, num_experts):
    """(offsets int32 [E + 1], dest int32 [T, topk], token_of_row int32 [R], R) for expert ids [T, topk]: a
    stable sort of the flat ids, per-expert counts rounded up to 64, their running sum. All on the device."""
    T, topk = expert_ids.shape
    E, n = num_experts, T * topk
    R = (n + 63) // 64 * 64 + 64 * E
    flat = expert_ids.reshape(-1).long()
    dev = flat.device
    order = torch.argsort(flat, stable=True)
    counts = torch.zeros(E, dtype=torch.long, device=dev).scatter_add_(0, flat, torch.ones_like(flat))
    ends = torch.cumsum((counts + 63) // 64 * 64, 0)
    offsets = torch.cat([ends.new_zeros(1), ends])
    sorted_e = flat[order]
    first = torch.cumsum(counts, 0) - counts               # position of each expert's first row in the sort
    row = offsets[sorted_e] + torch.arange(n, device=dev) - first[sorted_e]
    dest = torch.empty(n, dtype=torch.int32, device=dev)
    dest[order] = row.int()
    token_of_row = torch.full((R,), -1, dtype=torch.int32, device=dev)
    token_of_row[row] = (order // topk).int()
    return offsets.int(), dest.view(T, topk), token_of_row, R


def _native_maps(expert_ids, num_experts):
    return (_ext.use_native(expert_ids) and expert_ids.dtype in (torch.int32, torch.int64)
            and expert_ids.is_contiguous() and expert_ids.numel() > 0
            and _ext.require().moe_route_supported(expert_ids.shape[0], num_experts, expert_ids.shape[1], torch.float32))


def _maps(expert_ids, num_experts):
    """(offsets, dest, token_of_row) of ``_routing_maps``, on supported device ids by the hist, scan and place
    kernels of csrc/moe_route.hip instead of the sort: the same tensors, bit for bit."""
    if _native_maps(expert_ids, num_experts):
        return tuple(_ext.require().moe_route_maps(expert_ids, num_experts)[:3])
    return _routing_maps(expert_ids, num_experts)[:3]


# ---------------------------------------------------------------------------
# routing
class Routing(NamedTuple):
    """What :func:`moe_route` returns. ``R = round_up(T * topk, 64) + 64 * E``."""
    probs: torch.Tensor               # fp32 [T, topk]: softmax over the chosen logits, descending (sigmoid: rule 5)
    expert_ids: torch.Tensor          # int32 [T, topk]
    tokens_per_expert: torch.Tensor   # int32 [E]
    offsets: torch.Tensor             # int32 [E + 1], the segment table of the module docstring
    dest: torch.Tensor                # int32 [T, topk]: the row of token t's copy for its k-th expert
    token_of_row: torch.Tensor        # int32 [R]: the token of every row, -1 on pad and tail rows
    row_prob: torch.Tensor            # fp32 [R]: probs[t, k] at dest[t, k], 0 elsewhere (detached)
    aux_loss: Optional[torch.Tensor]  # 0-dim fp32, or None


def moe_route_supported(T, E, topk, dtype):
    """Can the routing kernels take ``[T, E]`` logits of ``dtype``? fp32 / fp16 / bf16, ``1 <= topk <= 8``, ``topk
    <= E <= 256``, ``T >= 1`` and ``T * topk + 64 * E < 2**31``. Needs the built extension."""
    return bool(_ext.require().moe_route_supported(int(T), int(E), int(topk), dtype))


def _aux_scale(T, E, topk):
    return E / (T * T * topk)


def _route_reference(logits, topk, aux_loss):
    """The PyTorch formulation: a stable descending sort (ties to the lowest expert index), a softmax over the
    first ``topk`` columns, ``_routing_maps``."""
    T, E = logits.shape
    lf = logits.float()
    top, idx = torch.sort(lf, dim=-1, descending=True, stable=True)
    ids = idx[:, :topk].contiguous()
    probs = torch.softmax(top[:, :topk], dim=-1)
    offsets, dest, token_of_row, R = _routing_maps(ids, E)
    flat = ids.reshape(-1)
    counts = torch.zeros(E, dtype=torch.long, device=ids.device).scatter_add_(0, flat, torch.ones_like(flat))
    row_prob = torch.zeros(R, dtype=torch.float32, device=ids.device).scatter_(
        0, dest.reshape(-1).long(), probs.detach().reshape(-1))
    aux = None
    if aux_loss:
        aux = _aux_scale(T, E, topk) * (counts.float() * torch.softmax(lf, dim=-1).sum(0)).sum()
    return Routing(probs, ids.int(), counts.int(), offsets, dest, token_of_row, row_prob, aux)


def _sigmoid_reference(logits, topk, aux_loss, expert_bias, num_groups, group_topk, scaling_factor):
    """The PyTorch formulation of the sigmoid router (the seven rules of :func:`moe_route`): stable descending
    sorts for the groups and the experts, so ties go to the lowest index; nothing is read on the host."""
    T, E = logits.shape
    lf = logits.float()
    s = torch.sigmoid(torch.where(lf != lf, torch.full_like(lf, float("-inf")), lf))
    key = s.detach() if expert_bias is None else s.detach() + expert_bias.float()
    if num_groups:
        top2 = key.view(T, num_groups, E // num_groups).topk(2, dim=-1).values
        kept = torch.sort(top2[..., 0] + top2[..., 1], dim=-1, descending=True, stable=True).indices[:, :group_topk]
        mask = torch.zeros(T, num_groups, dtype=torch.bool, device=key.device).scatter_(1, kept, True)
        key = key.masked_fill(~mask.repeat_interleave(E // num_groups, dim=1), float("-inf"))
    ids = torch.sort(key, dim=-1, descending=True, stable=True).indices[:, :topk].contiguous()
    probs = scaling_factor * s.gather(1, ids)
    if topk > 1:
        probs = probs / (s.gather(1, ids).sum(-1, keepdim=True) + 1e-20)
    offsets, dest, token_of_row, R = _routing_maps(ids, E)
    flat = ids.reshape(-1)
    counts = torch.zeros(E, dtype=torch.long, device=ids.device).scatter_add_(0, flat, torch.ones_like(flat))
    row_prob = torch.zeros(R, dtype=torch.float32, device=ids.device).scatter_(
        0, dest.reshape(-1).long(), probs.detach().reshape(-1))
    aux = None
    if aux_loss:
        aux = _aux_scale(T, E, topk) * (counts.float() * (s / (s.sum(-1, keepdim=True) + 1e-20)).sum(0)).sum()
    return Routing(probs, ids.int(), counts.int(), offsets, dest, token_of_row, row_prob, aux)


class _Route(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, topk, aux_loss, score_function="softmax", expert_bias=None, num_groups=0, group_topk=0,
                scaling_factor=1.0):
        probs, ids, counts, offsets, dest, token_of_row, row_prob, aux = _ext.require().moe_route_fwd(
            logits, topk, aux_loss, score_function=score_function, expert_bias=expert_bias, num_groups=num_groups,
            group_topk=group_topk, scaling_factor=scaling_factor)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(logits, ids, probs, counts)
        ctx.router = (score_function, scaling_factor)
        ctx.mark_non_differentiable(ids, counts, offsets, dest, token_of_row, row_prob)
        return probs, ids, counts, offsets, dest, token_of_row, row_prob, aux   # aux: None without aux_loss

    @staticmethod
    def backward(ctx, dprobs, *rest):
        logits, ids, probs, counts = ctx.saved_tensors
        d_aux = rest[-1]
        if dprobs is not None:
            dprobs = dprobs.float().contiguous()
        if d_aux is not None:
            d_aux = d_aux.float().reshape(1).contiguous()
        dlogits = _ext.require().moe_route_bwd(logits, ids, probs, dprobs, counts, d_aux, score_function=ctx.router[0],
                                               scaling_factor=ctx.router[1])
        return (dlogits,) + (None,) * 7


def _check_sigmoid_options(E, topk, expert_bias, num_groups, group_topk, logits):
    if (num_groups is None) != (group_topk is None):
        raise ValueError("moe_route: num_groups and group_topk go together")
    if num_groups is not None:
        if not (1 <= num_groups <= 16 and E % num_groups == 0 and E // num_groups >= 2):
            raise ValueError(f"moe_route: num_groups={num_groups} must be in [1, 16], divide E={E} and leave two "
                             "experts per group")
        if not 1 <= group_topk <= num_groups:
            raise ValueError(f"moe_route: group_topk={group_topk} must be in [1, num_groups={num_groups}]")
        if topk > group_topk * (E // num_groups):
            raise ValueError(f"moe_route: topk={topk} exceeds the {group_topk * (E // num_groups)} experts of "
                             f"{group_topk} groups")
    if expert_bias is not None and (expert_bias.shape != (E,) or expert_bias.dtype != torch.float32
                                    or expert_bias.device != logits.device):
        raise ValueError("moe_route: expert_bias must be an fp32 [E] tensor on logits' device")


def moe_route(logits, topk, aux_loss=False, fused=None, *, score_function="softmax", expert_bias=None,
              num_groups=None, group_topk=None, scaling_factor=1.0):
    """Route tokens to their ``topk`` experts. ``logits [T, E]`` (fp32, fp16 or bf16; used in fp32). Returns a
    :class:`Routing`: ``expert_ids`` are the ``topk`` largest logits of every token in descending order, equal
    logits going to the lowest expert index; ``probs`` the softmax over those ``topk`` logits; ``offsets``,
    ``dest`` and ``token_of_row`` the row maps :func:`moe_permute` builds for these ids, so passing the routing
    to it and to :func:`moe_unpermute` launches no index op. With ``aux_loss`` the Switch / Megatron
    load-balancing loss with coefficient 1, ``E / (T * T * topk) * sum_e tokens_per_expert[e] * sum_t
    softmax(logits)[t, e]``, the counts being constants of its gradient. Differentiable in ``logits`` through
    ``probs`` and ``aux_loss``.

    Device logits within ``moe_route_supported`` run csrc/moe_route.hip: three launches forward, one backward,
    no atomics, nothing read on the host, bit-reproducible. CPU tensors, ``APEX_FORCE_REFERENCE=1`` and other
    shapes take a stable sort in PyTorch with the same outputs. ``fused``: None takes the kernels where they
    were measured faster (``E < 64`` or ``topk <= 2``), True insists on them, False on the PyTorch path.

    ``score_function="sigmoid"`` is the router of the wide top-8 models (DeepSeek-V3; Megatron-Core's
    ``moe_router_score_function`` and its companions), and the only one that takes the other four options:

    1. the score is ``s = sigmoid(logits)``;
    2. the key ``s + expert_bias`` (a finite fp32 ``[E]`` constant; without one the key is ``s``) decides the
       selection and nothing else;
    3. with ``num_groups = G`` expert ``e`` is in group ``e // (E / G)`` (``E % G == 0``, ``E / G >= 2``, ``G <=
       16``), a group's score is the sum of its two largest keys, and only the experts of the ``group_topk``
       groups with the largest scores (ties to the lowest group) can be chosen; ``topk <= group_topk * E / G``;
    4. ``expert_ids`` are the ``topk`` eligible experts with the largest keys, descending, ties to the lowest index;
    5. ``probs = scaling_factor * s / (sum of the chosen s + 1e-20)``, and ``scaling_factor * s`` for ``topk == 1``;
    6. ``aux_loss`` takes ``s / (sum_e s + 1e-20)`` in place of the softmax;
    7. the row maps and the gradients are as above; experts a token did not choose get an exactly zero gradient
       from ``probs``.

    Its kernels (same file, same three-plus-one launches) split the work for wide ``E``, and ``fused=None`` takes
    them wherever they are supported: they were measured faster at every shape timed."""
    if logits.dim() != 2 or not 1 <= topk <= logits.shape[1]:
        raise ValueError(f"moe_route: logits [T, E] and 1 <= topk <= E, got {tuple(logits.shape)} and topk={topk}")
    if score_function not in ("softmax", "sigmoid"):
        raise ValueError(f"moe_route: score_function must be 'softmax' or 'sigmoid', got {score_function!r}")
    sigmoid = score_function == "sigmoid"
    if not sigmoid and (expert_bias is not None or num_groups is not None or group_topk is not None
                        or scaling_factor != 1.0):
        raise ValueError("moe_route: expert_bias, num_groups, group_topk and scaling_factor need "
                         "score_function='sigmoid'")
    native = _ext.use_native(logits) and logits.dtype in (torch.float32,) + _HALF and logits.numel() > 0 \
        and moe_route_supported(logits.shape[0], logits.shape[1], topk, logits.dtype)
    if fused and not native:
        raise ValueError("moe_route: fused=True needs device logits within moe_route_supported")
    if sigmoid:
        _check_sigmoid_options(logits.shape[1], topk, expert_bias, num_groups, group_topk, logits)
        opts = (None if expert_bias is None else expert_bias.detach().contiguous(), int(num_groups or 0),
                int(group_topk or 0), float(scaling_factor))
        if fused is None:
            # profiles/moe_route_sigmoid_vs_torch.jsonl: the kernels are faster than the PyTorch formulation at
            # every shape timed (T = 4096 / 16384, E = 8 / 64 / 128 / 256, topk = 2 / 4 / 8, with and without
            # groups, forward and forward + backward; by 1.5x at the least), so wherever they are supported
            fused = native
        if fused:
            return Routing(*_Route.apply(logits.contiguous(), int(topk), bool(aux_loss), "sigmoid", *opts))
        return _sigmoid_reference(logits, int(topk), bool(aux_loss), *opts)
    if fused is None:
        # profiles/moe_route_vs_torch.jsonl: with one token per wave pass (E >= 64) the kernels lose to the
        # PyTorch formulation at topk = 8 and win at topk = 2; nothing between was measured
        fused = native and (logits.shape[1] < 64 or topk <= 2)
    if fused:
        return Routing(*_Route.apply(logits.contiguous(), int(topk), bool(aux_loss)))
    return _route_reference(logits, int(topk), bool(aux_loss))


class _Permute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dest, token_of_row):
        ctx.save_for_backward(dest)
        return _gather(x, token_of_row)

    @staticmethod
    def backward(ctx, dxp):
        (dest,) = ctx.saved_tensors
        return _combine(dxp, dest)[0], None, None


class _Unpermute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, yp, dest, probs, token_of_row, row_prob):
        w = None if probs is None else probs.float().contiguous()
        ctx.save_for_backward(yp, dest, w, token_of_row, row_prob)
        ctx.pdtype = None if probs is None else probs.dtype
        return _combine(yp, dest, w)[0]

    @staticmethod
    def backward(ctx, dout):
        yp, dest, w, token_of_row, scale = ctx.saved_tensors
        R, (T, topk) = yp.shape[0], dest.shape
        dyp = dw = None
        if ctx.needs_input_grad[0]:
            if token_of_row is None:   # no routing given: rebuild the row maps from dest
                flat = dest.reshape(-1).long()
                token_of_row = torch.full((R,), -1, dtype=torch.int32, device=yp.device)
                token_of_row[flat] = (torch.arange(T * topk, device=yp.device) // topk).int()
                scale = None if w is None else torch.zeros(R, dtype=torch.float32, device=yp.device).scatter_(
                    0, flat, w.reshape(-1))
            dyp = _gather(dout, token_of_row, scale)
        if w is not None and ctx.needs_input_grad[2]:
            dw = _combine(yp, dest, None, dout, want_out=False)[1].to(ctx.pdtype)
        return dyp, None, dw, None, None


def moe_permute(x, expert_ids, num_experts, routing=None):
    """Sort tokens by expert. ``x [T, H]``, ``expert_ids [T, topk]`` integers in ``[0, num_experts)``. Returns
    ``(xp, offsets, dest)``: ``xp [R, H]`` in the segment layout of the module docstring, with ``R = round_up(T * topk, 64) + 64 * num_experts`` and every pad and tail row zero;
    ``offsets`` int32 ``[num_experts + 1]``; ``dest`` int32 ``[T, topk]``, the row of ``xp`` that holds token
    ``t``'s copy for its ``k``-th expert (``xp[dest[t, k]]`` is bit-equal to ``x[t]``). Differentiable in ``x``;
    nothing is read on the host. ``routing``: the :class:`Routing` that :func:`moe_route` returned with these
    ``expert_ids``; its maps are used as they are and no index op is launched."""
    if x.dim() != 2 or expert_ids.dim() != 2 or expert_ids.shape[0] != x.shape[0]:
        raise ValueError(f"moe_permute: x [T, H] and expert_ids [T, topk], got {tuple(x.shape)} and "
                         f"{tuple(expert_ids.shape)}")
    if routing is not None:
        if routing.dest.shape != expert_ids.shape or routing.offsets.numel() != num_experts + 1:
            raise ValueError("moe_permute: routing does not belong to these expert_ids")
        offsets, dest, token_of_row = routing.offsets, routing.dest, routing.token_of_row
    else:
        offsets, dest, token_of_row = _maps(expert_ids, num_experts)
    return _Permute.apply(x, dest, token_of_row), offsets, dest


def moe_unpermute(yp, dest, probs=None, routing=None):
    """``out[t] = sum_k probs[t, k] * yp[dest[t, k]]`` for ``yp [R, H]`` and ``dest`` from :func:`moe_permute`;
    fp32 accumulation in the order ``k = 0, 1, ...``, rounded once. ``probs [T, topk]`` (any float dtype, used in
    fp32) or None for a plain sum. Differentiable in ``yp`` and ``probs``. ``routing``: the :class:`Routing`
    that ``dest`` and ``probs`` (its ``probs``, or None) come from; the backward then reads its ``token_of_row``
    and ``row_prob`` instead of rebuilding them from ``dest``."""
    if yp.dim() != 2 or dest.dim() != 2 or (probs is not None and probs.shape != dest.shape):
        raise ValueError("moe_unpermute: yp [R, H], dest [T, topk] and probs [T, topk] or None")
    if routing is None:
        return _Unpermute.apply(yp, dest, probs, None, None)
    if routing.token_of_row.numel() != yp.shape[0]:
        raise ValueError("moe_unpermute: routing does not belong to yp")
    return _Unpermute.apply(yp, dest, probs, routing.token_of_row, None if probs is None else routing.row_prob)
