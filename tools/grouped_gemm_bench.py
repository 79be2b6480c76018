"""Grouped MoE GEMMs (csrc/gemm_grouped.hip, through apex.ops.grouped_linear) against the per-expert loop of
torch.matmul on host-known slices (profiles/grouped_gemm_vs_loop.jsonl).

usage: python tools/grouped_gemm_bench.py OUT.jsonl [--samples 7] [--iters 10]   (rows are appended)

Shapes: 16384 routed rows over E = 8 experts, K = 2560, N = 2 * 6912 (a gated first expert GEMM), balanced and
skewed (one expert holds half the rows); and E = 64 experts of 256 rows. Per shape and per pass (forward, input
gradient, weight gradient) the grouped launch and the loop are sampled in turn, round after round, in one
process, so a clock drift or a neighbour on the host lands on both alike; a sample is `iters` calls between two
device events; the graphics clock is sampled while the rounds run. The loop is given the segment boundaries as
Python integers, which a real step would have to read back from the device every layer (a sync the grouped
path does not have and these timings do not charge); its weight gradient writes [E, N, K] slices in place and
its input gradient uses W in place (no transposed copy), while the grouped input gradient is timed with its
per-step transposed copy of the weights, as grouped_linear runs it (grouped_dgrad_kernel_only: the same
launch on a copy made beforehand). Reported: median / min / max microseconds and
TFLOP/s (2 rows N K over the median). The first row of a run records the command line.
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
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()

    from apex import _ext
    from apex.utils.telemetry import GpuSampler

    C = _ext.require()
    dev = "cuda"
    lines = [dict(what="command", argv=["tools/grouped_gemm_bench.py"] + sys.argv[1:],
                  device=torch.cuda.get_device_name(0))]

    def sample(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters

    def run(variants, extra, flops):
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
            med = statistics.median(times[k])
            lines.append(dict(what=k, **extra, us_median=round(med, 2), us_min=round(min(times[k]), 2),
                              us_max=round(max(times[k]), 2), tflops=round(flops / med / 1e6, 1),
                              samples=args.samples, iters=args.iters, sclk_mhz=clock))
            print(json.dumps(lines[-1]), flush=True)

    K, N = 2560, 2 * 6912
    shapes = [("e8_balanced", [2048] * 8, K, N), ("e8_skewed", [8192] + [1152] * 6 + [1280], K, N),
              ("e64_x256", [256] * 64, K, N)]
    for name, rows, K, N in shapes:
        E, total = len(rows), sum(rows)
        R = total + 64 * E                      # moe_permute's static bound: the rest is tail
        off = [sum(rows[:i]) for i in range(E + 1)]
        torch.manual_seed(0)
        x = (torch.randn(R, K, device=dev) * 0.05).bfloat16()
        w = (torch.randn(E, N, K, device=dev) * 0.05).bfloat16()
        dy = (torch.randn(R, N, device=dev) * 0.05).bfloat16()
        x[total:], dy[total:] = 0, 0
        offsets = torch.tensor(off, dtype=torch.int32, device=dev)
        y, dx, dw = torch.empty(R, N, device=dev).bfloat16(), torch.empty_like(x), torch.empty_like(w)
        seg = [slice(off[e], off[e + 1]) for e in range(E)]

        def loop_fwd():
            for e in range(E):
                torch.matmul(x[seg[e]], w[e].t(), out=y[seg[e]])

        def loop_dgrad():
            for e in range(E):
                torch.matmul(dy[seg[e]], w[e], out=dx[seg[e]])

        def loop_wgrad():
            for e in range(E):
                torch.matmul(dy[seg[e]].t(), x[seg[e]], out=dw[e])

        loop_fwd(), loop_dgrad(), loop_wgrad()
        g_y = C.gemm_grouped_nt(x, w, offsets)
        g_dx = C.gemm_grouped_nt(dy, w.transpose(1, 2).contiguous(), offsets)
        g_dw = C.gemm_grouped_tt(dy, x, offsets)
        rel = lambda a, b: round(float((a.float() - b.float()).norm() / b.float().norm()), 6)  # noqa: E731
        extra = dict(shape=name, E=E, rows=total, R=R, K=K, N=N,
                     rel_diff_vs_loop=dict(fwd=rel(g_y[:total], y[:total]), dgrad=rel(g_dx[:total], dx[:total]),
                                           wgrad=rel(g_dw, dw)))
        flops = 2.0 * total * N * K
        run({"grouped_fwd": lambda: C.gemm_grouped_nt(x, w, offsets), "loop_fwd": loop_fwd}, extra, flops)
        wt = w.transpose(1, 2).contiguous()
        run({"grouped_dgrad": lambda: C.gemm_grouped_nt(dy, w.transpose(1, 2).contiguous(), offsets),
             "grouped_dgrad_kernel_only": lambda: C.gemm_grouped_nt(dy, wt, offsets),   # W^T made beforehand
             "loop_dgrad": loop_dgrad}, extra, flops)
        del wt
        run({"grouped_wgrad": lambda: C.gemm_grouped_tt(dy, x, offsets), "loop_wgrad": loop_wgrad}, extra, flops)
        del x, w, dy, y, dx, dw, g_y, g_dx, g_dw
    with open(args.out, "a") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
