#!/usr/bin/env python3
"""Fused RoPE on packed QKV (apply_rotary_qkv_packed, csrc/rope.hip) against the eager composition
(the module's reference function on device tensors), bf16, forward and forward + backward.

Both arms run in ONE process on the same random data, alternating round by round; every round is
timed with device events around ``--iters`` back-to-back calls. One JSON line per (shape, pass):
median / min time per call of both arms, the speed-up, and the fused arm's achieved bytes/s from
the algorithmic traffic (read + write of the packed tensor plus the two fp32 tables, per
direction) with its share of the MI355X HBM peak (8.0 TB/s spec; 6.29 TB/s is what a float4 copy
reaches). Tensors smaller than the 256 MB last-level cache can exceed the HBM figure.

  python benchmarks/rope.py [--rounds 10] [--iters 10] [--out profiles/rope_kernel_vs_composition.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC = 8.0e12
HBM_COPY = 6.29e12

# (name, [B, S, 3, h, d]): benchmarks/megatron_gpt.py defaults (hidden 2560, 20 heads of 128, seq 2048,
# micro-batch 4; 5 rank-local heads at the default TP = 4, 20 at TP = 1) and GPT-2 1.5B (25 heads of
# 64, seq 1024) at benchmarks/gpt2.py's per-GPU batch 16
SHAPES = [("megatron_gpt tp4 (default)", (4, 2048, 3, 5, 128)),
          ("megatron_gpt tp1", (4, 2048, 3, 20, 128)),
          ("gpt2 1.5b b16", (16, 1024, 3, 25, 64))]


def traffic_bytes(shape, d2, backward):
    B, S, _, h, d = shape
    one = 2 * (B * S * 3 * h * d * 2) + 2 * S * d2 * 4  # read + write bf16, cos + sin fp32
    return one * (2 if backward else 1)


def time_rounds(arms, rounds, iters, warmup):
    """arms: {name: fn}. Alternates the arms every round; returns {name: [seconds per call]}."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {n: [] for n in arms}
    for _ in range(rounds):
        for n, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            out[n].append(e0.elapsed_time(e1) * 1e-3 / iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed round (rounds x iters >= 50 per arm)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.rounds * args.iters < 50:
        ap.error("rounds x iters must be at least 50 per arm")

    from apex.utils.bench import init_distributed, log, protect_stdout

    if not torch.cuda.is_available():
        sys.exit("benchmarks/rope.py measures on the GPU; no device found")
    env = init_distributed()
    stream = protect_stdout()

    import apex
    from apex.transformer.functional import fused_rope as fr

    apex._ext.require()
    lines = []
    for name, shape in SHAPES:
        B, S, _, h, d = shape
        g = torch.Generator(device=env.device).manual_seed(0)
        qkv = torch.randn(shape, device=env.device, generator=g).to(torch.bfloat16).requires_grad_(True)
        dy = torch.randn(shape, device=env.device, generator=g).to(torch.bfloat16)
        cos, sin = fr.RotaryEmbedding(d).cos_sin(S, device=env.device)
        # same results first (bf16: both round an fp32 result once)
        with torch.no_grad():
            a, b = fr.apply_rotary_qkv_packed(qkv, cos, sin), fr.rope_reference_qkv_packed(qkv, cos, sin)
            max_diff = float((a.float() - b.float()).abs().max())
            del a, b

        def fwd(f):
            def run():
                with torch.no_grad():
                    f(qkv, cos, sin)
            return run

        def fwd_bwd(f):
            def run():
                torch.autograd.grad(f(qkv, cos, sin), qkv, dy)
            return run

        for pass_, wrap in (("fwd", fwd), ("fwd+bwd", fwd_bwd)):
            t = time_rounds({"fused": wrap(fr.apply_rotary_qkv_packed),
                             "composition": wrap(fr.rope_reference_qkv_packed)},
                            args.rounds, args.iters, args.warmup)
            med = {n: statistics.median(v) for n, v in t.items()}
            nbytes = traffic_bytes(shape, d, pass_ != "fwd")
            bw = nbytes / med["fused"]
            line = {"bench": "rope_kernel_vs_composition", "shape": name, "qkv": list(shape), "dtype": "bf16",
                    "pass": pass_, "rounds": args.rounds, "iters_per_round": args.iters,
                    "fused_us_median": round(med["fused"] * 1e6, 2),
                    "fused_us_min": round(min(t["fused"]) * 1e6, 2),
                    "composition_us_median": round(med["composition"] * 1e6, 2),
                    "composition_us_min": round(min(t["composition"]) * 1e6, 2),
                    "speedup_median": round(med["composition"] / med["fused"], 2),
                    "algorithmic_bytes": nbytes,
                    "fused_tb_per_s": round(bw / 1e12, 3),
                    "share_of_hbm_spec_8.0": round(bw / HBM_SPEC, 3),
                    "share_of_hbm_copy_6.29": round(bw / HBM_COPY, 3),
                    "tensor_mb": round(B * S * 3 * h * d * 2 / 2 ** 20, 1),
                    "max_abs_diff_vs_composition": max_diff,
                    "timing": "device events around iters back-to-back calls of the Python op "
                              "(host launch cost included)"}
            lines.append(line)
            log(json.dumps(line))
        del qkv, dy
    for line in lines:
        print(json.dumps(line), file=stream, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
