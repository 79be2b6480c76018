"""Per-call flash-attention timings against one built apex._C (loaded by path, so two builds can be
compared from one checkout by running this once per build, alternating; profiles/gqa_attn_ab.jsonl).

usage: python tools/gqa_bench.py PATH_TO__C.so LABEL OUT.jsonl   (rows are appended to OUT.jsonl)
  mha_fwd / mha_bwd    B=768 S=128 H=16 D=64 bf16 dropout 0.1 (the BERT bench shape), per call
  gqa_compose_fwd_bwd  B=4 S=2048 H=32 Hk=8 D=128 causal bf16: repeat_interleave + MHA kernels + group
                       sum of dK / dV (what a user writes without grouped-query kernels)
  gqa_new_fwd_bwd      the same shape through the grouped kernels, scratch and reduction included
  gqa_reduce_only      attn_kv_group_reduce alone
The gqa_new rows need a build that has the grouped-query kernels; other builds skip them.
"""
import importlib.util
import json
import math
import statistics
import sys

import torch

path, label, out = sys.argv[1:4]
spec = importlib.util.spec_from_file_location("_C", path)
C = importlib.util.module_from_spec(spec)
spec.loader.exec_module(C)
dev = "cuda"
has_gqa = hasattr(C, "attn_kv_group_reduce")


def timed(fn, iters, windows=7, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b) * 1e3 / iters)
    return dict(us_median=round(statistics.median(res), 2), us_min=round(min(res), 2), us_max=round(max(res), 2),
                iters=iters, windows=windows)


rows = []


def emit(name, **kw):
    r = dict(label=label, what=name, **kw)
    rows.append(r)
    print(json.dumps(r), flush=True)


# ---------------------------------------------------------------- MHA at the bench shape
torch.manual_seed(0)
B, S, H, D, p = 768, 128, 16, 64, 0.1
qkv = (torch.randn(B, S, 3, H, D, device=dev) * 0.8).bfloat16()
q, k, v = qkv.unbind(2)
scale = 1 / math.sqrt(D)
o, lse, dmask = C.flash_attn_fwd(q, k, v, False, scale, p, 1, 2, None)
do = torch.randn_like(o)
dqkv = torch.empty_like(qkv)
dq, dk, dv = dqkv.unbind(2)
emit("mha_fwd", shape=[B, S, H, D], **timed(lambda: C.flash_attn_fwd(q, k, v, False, scale, p, 1, 2, None), 50))
emit("mha_bwd", shape=[B, S, H, D],
     **timed(lambda: C.flash_attn_bwd(do, q, k, v, o, lse, dq, dk, dv, False, scale, p, 1, 2, None, dmask), 50))
del qkv, q, k, v, o, lse, dmask, do, dqkv, dq, dk, dv

# ---------------------------------------------------------------- GQA shape
B, S, H, Hk, D = 4, 2048, 32, 8, 128
g = H // Hk
scale = 1 / math.sqrt(D)
q = (torch.randn(B, S, H, D, device=dev) * 0.8).bfloat16()
k = (torch.randn(B, S, Hk, D, device=dev) * 0.8).bfloat16()
v = (torch.randn(B, S, Hk, D, device=dev) * 0.8).bfloat16()
do = torch.randn_like(q)


def compose():
    ke, ve = k.repeat_interleave(g, dim=2), v.repeat_interleave(g, dim=2)
    o, lse, dmask = C.flash_attn_fwd(q, ke, ve, True, scale, 0.0, 0, 0, None)
    dq, dke, dve = torch.empty_like(q), torch.empty_like(ke), torch.empty_like(ve)
    C.flash_attn_bwd(do, q, ke, ve, o, lse, dq, dke, dve, True, scale, 0.0, 0, 0, None, dmask)
    dk = dke.view(B, S, Hk, g, D).sum(3)
    dv = dve.view(B, S, Hk, g, D).sum(3)
    return o, dq, dk, dv


def grouped():
    o, lse, dmask = C.flash_attn_fwd(q, k, v, True, scale, 0.0, 0, 0, None)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    C.flash_attn_bwd(do, q, k, v, o, lse, dq, dk, dv, True, scale, 0.0, 0, 0, None, dmask)
    return o, dq, dk, dv


shape = [B, S, H, Hk, D]
emit("gqa_compose_fwd_bwd", shape=shape, **timed(compose, 10))
if has_gqa:
    emit("gqa_new_fwd_bwd", shape=shape, **timed(grouped, 10))
    dk_x, dv_x = torch.randn(B, S, H, D, device=dev).bfloat16(), torch.randn(B, S, H, D, device=dev).bfloat16()
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    emit("gqa_reduce_only", shape=shape, scratch_bytes=2 * dk_x.numel() * 2,
         **timed(lambda: C.attn_kv_group_reduce(dk_x, dv_x, dk, dv), 20))
    # same results (the composition sums the group in another order and precision)
    a, b = grouped(), compose()
    emit("gqa_new_vs_compose", o_equal=bool(torch.equal(a[0], b[0])), dq_equal=bool(torch.equal(a[1], b[1])),
         dk_max_abs_diff=float((a[2].float() - b[2].float()).abs().max()),
         dv_max_abs_diff=float((a[3].float() - b[3].float()).abs().max()),
         dk_max_abs=float(b[2].float().abs().max()))
with open(out, "a") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
