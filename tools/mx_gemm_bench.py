"""MXFP8 GEMM (csrc/gemm_mx.hip) against the per-tensor fp8 GEMM and the bf16 GEMM of csrc/gemm.hip, and the
MX quantiser's throughput (profiles/mx_gemm_vs_f8.jsonl).

usage: python tools/mx_gemm_bench.py OUT.jsonl [--m 98304] [--samples 7] [--iters 20]   (rows are appended)

BERT-Large's four layer shapes at M tokens, bf16 output, no epilogue. Per shape the three GEMMs are sampled in
turn, round after round, in one process, so a clock drift or a neighbour on the host lands on all alike; a
sample is `iters` calls between two device events; the graphics clock is sampled while the rounds run. Reported:
median / min / max microseconds and TFLOP/s (2 M N K over the median). The quantiser rows time mx_quantize of the
[M, K] bf16 activation rowwise, colwise and both, with the bytes it has to move (2 bytes read, 1 + 1/32 written
per element and orientation) over the median. The first row of a run records the command line.
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
    ap.add_argument("--m", type=int, default=98304)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()

    import apex.fp8 as fp8
    from apex import _ext
    from apex.utils.telemetry import GpuSampler

    C = _ext.require()
    M, dev = args.m, "cuda"
    lines = [dict(what="command", argv=["tools/mx_gemm_bench.py"] + sys.argv[1:], device=torch.cuda.get_device_name(0))]
    one = torch.ones(1, device=dev)

    def sample(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters

    def run(variants, extra):
        for fn, _ in variants.values():   # warm every shape of the timed window
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        sampler = GpuSampler(0, period=0.02).start()
        for _ in range(args.samples):     # interleaved: one sample of each variant per round
            for k, (fn, _) in variants.items():
                times[k].append(sample(fn))
        clock = (sampler.stop() or {}).get("sclk_mhz")
        for k, (_, rate) in variants.items():
            med = statistics.median(times[k])
            lines.append(dict(what=k, **extra, us_median=round(med, 2), us_min=round(min(times[k]), 2),
                              us_max=round(max(times[k]), 2), **rate(med), samples=args.samples, iters=args.iters,
                              sclk_mhz=clock))
            print(json.dumps(lines[-1]), flush=True)

    for name, N, K in [("qkv", 3072, 1024), ("attn_out", 1024, 1024), ("fc1", 4096, 1024), ("fc2", 1024, 4096)]:
        torch.manual_seed(0)
        a = torch.randn(M, K, device=dev).bfloat16()
        w = (torch.randn(N, K, device=dev) * 0.05).bfloat16()
        a8, w8 = C.fp8_quantize(a, 0, one * 64), C.fp8_quantize(w, 0, one * 1024)
        (am, asc), (wm, wsc) = fp8.mx_quantize(a), fp8.mx_quantize(w)
        flops = 2.0 * M * N * K
        tf = lambda us: dict(tflops=round(flops / us / 1e6, 1))  # noqa: E731
        # the MX product is the bf16 product up to the quantisation of both operands
        ref = C.gemm(a, w, C.EPI_NONE)[0].float()
        got = fp8.mx_gemm(am, asc, wm, wsc).float()
        rel = float((got - ref).norm() / ref.norm())
        run({"mx_gemm": (lambda: fp8.mx_gemm(am, asc, wm, wsc), tf),
             "gemm_f8": (lambda: C.gemm_f8(a8, w8, one, one, 0, C.EPI_NONE), tf),
             "gemm_bf16": (lambda: C.gemm(a, w, C.EPI_NONE), tf)},
            dict(shape=name, M=M, N=N, K=K, mx_rel_diff_vs_bf16=round(rel, 5)))
        del ref, got
        if name in ("qkv", "fc2"):  # the two activation widths
            gb = lambda n: (lambda us: dict(bytes=int(a.numel() * (2 + n * (1 + 1 / 32))),  # noqa: E731
                                            gbytes_per_s=round(a.numel() * (2 + n * (1 + 1 / 32)) / us / 1e3, 1)))
            run({"mx_quantize_row": (lambda: fp8.mx_quantize(a, 0, True, False), gb(1)),
                 "mx_quantize_col": (lambda: fp8.mx_quantize(a, 0, False, True), gb(1)),
                 "mx_quantize_both": (lambda: fp8.mx_quantize(a, 0, True, True), gb(2)),
                 "fp8_quantize": (lambda: C.fp8_quantize(a, 0, one), lambda us: dict(
                     bytes=a.numel() * 3, gbytes_per_s=round(a.numel() * 3 / us / 1e3, 1)))},
                dict(shape=f"act_{name}", M=M, K=K))
        del a, w, a8, w8, am, asc, wm, wsc
    with open(args.out, "a") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
