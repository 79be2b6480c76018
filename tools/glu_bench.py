"""Gated activation (SwiGLU): the fused HIP kernels against the PyTorch composition, and against this
project's own bias_act kernels at the same bytes moved (profiles/glu_bench.jsonl).

usage: python tools/glu_bench.py OUT.jsonl [--rows 16384] [--samples 9] [--iters 100]   (rows are appended)

rows = a GPT step's token count (16 x 1024), F = 4096 and 6400 (GPT-2 1.5B's 4 x 1600), bf16, with and
without a bf16 bias. Per (F, bias) the variants below are sampled in turn, round after round, in one
process, so a drift of the clock or a neighbour on the host lands on all of them alike; each sample
is `iters` calls between two device events. Reported per variant: the median, min and max of the samples in
microseconds, the bytes the algorithm has to move (computed here from the shape) over the median in GB/s, and
the graphics clock sampled while the round ran.

  glu_fwd / glu_bwd            apex._C.glu_fwd / glu_bwd (bwd with the bias gradient when there is a bias)
  compose_fwd / compose_bwd    chunk -> (+ bias) -> F.silu -> mul, and its autograd backward (forward excluded)
  bias_act_fwd / bias_act_bwd  apex._C.bias_act_* (tanh GELU) on [rows, C] with C chosen so that the bytes
                               equal the gated kernel's: fwd 2 C = 3 F, bwd 3 C = 5 F
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--rows", type=int, default=16 * 1024)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()

    from apex import _ext
    from apex.ops.fused import ACT_GELU_TANH, ACT_SILU
    from apex.utils.telemetry import GpuSampler

    C = _ext.require()
    dev, dt, esz = "cuda", torch.bfloat16, 2
    rows = args.rows
    lines = []

    def sample(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters

    for Fw in (4096, 6400):
        for with_bias in (False, True):
            torch.manual_seed(0)
            x = (torch.randn(rows, 2 * Fw, device=dev) * 2).to(dt)
            dy = torch.randn(rows, Fw, device=dev).to(dt)
            bias = torch.randn(2 * Fw, device=dev).to(dt) if with_bias else None
            # bias_act at equal bytes: fwd reads C and writes C (2 C = 3 F); bwd reads 2 C and writes C (3 C = 5 F)
            cf, cb = 3 * Fw // 2 // 8 * 8, 5 * Fw // 3 // 8 * 8
            xf, xb = torch.randn(rows, cf, device=dev).to(dt), torch.randn(rows, cb, device=dev).to(dt)
            dyb = torch.randn(rows, cb, device=dev).to(dt)
            bf = torch.randn(cf, device=dev).to(dt) if with_bias else None
            bb = torch.randn(cb, device=dev).to(dt) if with_bias else None
            xr = x.clone().requires_grad_(True)
            br = bias.clone().requires_grad_(True) if with_bias else None

            def compose_fwd(xx=x, b_=bias):
                g, u = (xx + b_ if b_ is not None else xx).chunk(2, -1)
                return F.silu(g) * u

            yc = compose_fwd(xr, br)   # graph kept: the backward alone is timed
            gin = [xr, br] if with_bias else [xr]
            variants = {
                "glu_fwd": (lambda: C.glu_fwd(x, bias, ACT_SILU), 3 * Fw),
                "compose_fwd": (compose_fwd, 3 * Fw),
                "bias_act_fwd": (lambda: C.bias_act_fwd(xf, bf, ACT_GELU_TANH), 2 * cf),
                "glu_bwd": (lambda: C.glu_bwd(dy, x, bias, ACT_SILU, with_bias), 5 * Fw),
                "compose_bwd": (lambda: torch.autograd.grad(yc, gin, dy, retain_graph=True), 5 * Fw),
                "bias_act_bwd": (lambda: C.bias_act_bwd(dyb, xb, bb, ACT_GELU_TANH), 3 * cb),
            }
            # the fused result is the composition's up to the roundings the composition adds
            yk = C.glu_fwd(x, bias, ACT_SILU)
            fwd_diff = float((yk.float() - compose_fwd().float()).abs().max())
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
            for k, (_, elems) in variants.items():
                med = statistics.median(times[k])
                nbytes = rows * elems * esz   # the algorithm's bytes (compose_*: the fused count, for comparison)
                lines.append(dict(what=k, rows=rows, F=Fw, bias=with_bias, dtype="bf16", us_median=round(med, 2),
                                  us_min=round(min(times[k]), 2), us_max=round(max(times[k]), 2),
                                  gbytes_per_s=round(nbytes / med / 1e3, 1), bytes=nbytes, samples=args.samples,
                                  iters=args.iters, sclk_mhz=clock, fwd_max_abs_diff_vs_compose=fwd_diff))
                print(json.dumps(lines[-1]), flush=True)
            del x, dy, xf, xb, dyb, xr, yc
    with open(args.out, "a") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
