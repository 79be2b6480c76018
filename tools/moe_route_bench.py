"""MoE routing plus row maps (csrc/moe_route.hip, through apex.ops.moe_route) against the PyTorch formulation it
replaces (profiles/moe_route_vs_torch.jsonl).

usage: python tools/moe_route_bench.py OUT.jsonl [--samples 7] [--iters 20]   (rows are appended)

Shapes: T in {4096, 16384} tokens, E in {8, 64, 256} experts, topk in {2, 8}, bf16 logits. One call is
moe_route(logits, topk, aux_loss=True, fused=True) (forward) or that plus the backward of (probs * g).sum() +
aux_loss (forward + backward). The PyTorch formulation is the same function on its reference path (fused=False:
a stable sort, softmax, _routing_maps), not a copy of it. Per shape the two variants
are sampled in turn, round after round, in one process, so a clock drift or a neighbour on the host lands on
both alike; a sample is `iters` calls between two device events; the graphics clock is sampled while the rounds
run. Reported: median / min / max microseconds per call. The first row of a run records the command line.

--router sigmoid times the sigmoid router instead (profiles/moe_route_sigmoid_vs_torch.jsonl): score_function=
"sigmoid" with an expert bias and scaling_factor 2.5, E in {8, 64, 128, 256}, topk in {2, 4, 8}, without groups and
(E >= 64) with num_groups = 8, group_topk = 4; the PyTorch formulation is again fused=False of the same call.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--router", choices=("softmax", "sigmoid"), default="softmax")
    args = ap.parse_args()

    from apex import _ext
    from apex.ops import moe_route
    from apex.utils.telemetry import GpuSampler

    _ext.require()
    lines = [dict(what="command", argv=["tools/moe_route_bench.py"] + sys.argv[1:],
                  device=torch.cuda.get_device_name(0))]

    def reference(fn):
        return lambda: fn(fused=False)

    def sample(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters

    def run(variants, extra):
        for fn in variants.values():   # warm every shape of the timed window
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        sampler = GpuSampler(0, period=0.02).start()
        for _ in range(args.samples):  # interleaved: one sample of each variant per round
            for k, fn in variants.items():
                times[k].append(sample(fn))
        clock = (sampler.stop() or {}).get("sclk_mhz")
        for k in variants:
            lines.append(dict(what=k, **extra, us_median=round(statistics.median(times[k]), 2),
                              us_min=round(min(times[k]), 2), us_max=round(max(times[k]), 2), samples=args.samples,
                              iters=args.iters, sclk_mhz=clock))
            print(json.dumps(lines[-1]), flush=True)

    sig = args.router == "sigmoid"
    for T in (4096, 16384):
        for E in (8, 64, 128, 256) if sig else (8, 64, 256):
            for topk, G in [(k, G) for k in ((2, 4, 8) if sig else (2, 8)) for G in ((None, 8) if sig and E >= 64 else (None,))]:
                torch.manual_seed(0)
                logits = torch.randn(T, E, device="cuda").bfloat16().requires_grad_()
                g = torch.randn(T, topk, device="cuda")
                kw = {}
                if sig:
                    kw = dict(score_function="sigmoid", scaling_factor=2.5, num_groups=G, group_topk=G and 4,
                              expert_bias=torch.randint(-4, 5, (E,), device="cuda").float() / 8)

                def fwd(fused=True):
                    return moe_route(logits, topk, aux_loss=True, fused=fused, **kw)

                def fwd_bwd(fused=True):
                    r = moe_route(logits, topk, aux_loss=True, fused=fused, **kw)
                    return torch.autograd.grad((r.probs * g).sum() + r.aux_loss, logits)

                a, b = fwd(), reference(fwd)()
                same = all(torch.equal(getattr(a, n), getattr(b, n)) for n in
                           ("expert_ids", "tokens_per_expert", "offsets", "dest", "token_of_row"))
                extra = dict(T=T, E=E, topk=topk, **(dict(router="sigmoid", num_groups=G) if sig else {}), maps_equal=same,
                             probs_max_diff=float((a.probs - b.probs).abs().max()))
                run({"fused_fwd": fwd, "torch_fwd": reference(fwd)}, extra)
                run({"fused_fwd_bwd": fwd_bwd, "torch_fwd_bwd": reference(fwd_bwd)}, extra)
    with open(args.out, "a") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
