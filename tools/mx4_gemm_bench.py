"""MXFP4 GEMMs (csrc/gemm_mx4.hip: fp8 x fp4, fp4 x fp4) against the MXFP8 GEMM (csrc/gemm_mx.hip), call times
(profiles/mx4_gemm_vs_mx8.jsonl).

usage: python tools/mx4_gemm_bench.py OUT.jsonl [--samples 7] [--iters 20]   (rows are appended)

8192^3 and BERT-Large's FFN shape at 98304 tokens (N = 4096, K = 1024), bf16 output, no epilogue. Per shape the
three products are sampled in turn, round after round, in one process; a sample is `iters` calls between two device
events (output allocation included: call time, not kernel time); the graphics clock is sampled while the rounds
run. Reported: median / min / max microseconds and TFLOP/s (2 M N K over the median), and each product's relative
difference from the bf16 GEMM of the unquantised operands on the same seeded inputs.
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
    args = ap.parse_args()

    import apex.fp8 as fp8
    from apex import _ext
    from apex.utils.telemetry import GpuSampler

    C = _ext.require()
    lines = [dict(what="command", argv=["tools/mx4_gemm_bench.py"] + sys.argv[1:], device=torch.cuda.get_device_name(0))]

    def sample(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters

    for name, M, N, K in [("8192^3", 8192, 8192, 8192), ("bert_fc1", 98304, 4096, 1024)]:
        torch.manual_seed(0)
        a = torch.randn(M, K, device="cuda").bfloat16()
        w = (torch.randn(N, K, device="cuda") * 0.05).bfloat16()
        a8, w8, a4, w4 = fp8.mx_quantize(a), fp8.mx_quantize(w), fp8.mx_quantize(a, "e2m1"), fp8.mx_quantize(w, "e2m1")
        variants = {"mx8_e4m3_e4m3": lambda: fp8.mx_gemm(*a8, *w8),
                    "mx4_e4m3_e2m1": lambda: fp8.mx_gemm(*a8, *w4, fp8.E4M3, fp8.E2M1),
                    "mx4_e2m1_e2m1": lambda: fp8.mx_gemm(*a4, *w4, fp8.E2M1, fp8.E2M1)}
        ref = C.gemm(a, w, C.EPI_NONE)[0].float()
        rel = {k: round(float((fn().float() - ref).norm() / ref.norm()), 5) for k, fn in variants.items()}
        del ref
        for fn in variants.values():      # warm every variant of the timed window
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        sampler = GpuSampler(0, period=0.02).start()
        for _ in range(args.samples):     # interleaved: one sample of each variant per round
            for k, fn in variants.items():
                times[k].append(sample(fn))
        clock = (sampler.stop() or {}).get("sclk_mhz")
        for k in variants:
            med = statistics.median(times[k])
            lines.append(dict(what=k, shape=name, M=M, N=N, K=K, us_median=round(med, 2), us_min=round(min(times[k]), 2),
                              us_max=round(max(times[k]), 2), tflops=round(2.0 * M * N * K / med / 1e6, 1),
                              rel_diff_vs_bf16=rel[k], samples=args.samples, iters=args.iters, sclk_mhz=clock))
            print(json.dumps(lines[-1]), flush=True)
        del a, w, a8, w8, a4, w4
    with open(args.out, "a") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
