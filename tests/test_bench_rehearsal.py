"""CPU/gloo rehearsal of bench.py's N-rank path (the driver's 2/4/8-GPU scaling runs).

``bench.py --cpu-rehearsal --full`` runs the SAME sequence the multi-GPU ``--full`` bench runs — pre-flight
known-value all-reduces, in-job bucket-size probe and selection, apex DDP with the chosen buckets,
warmup + timed steps bracketed by barriers, MAX over ranks, the fp32 pass, the all-reduce probe,
one JSON line from rank 0 — on CPU over gloo with a tiny BERT, launched exactly as the driver
launches it (``python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1``)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _plain_run(dump_dir):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cpu-rehearsal", "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(dump_dir)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """Without --full only the headline steps run (no fp32 / fp8 / fp16 pass, no all-reduce probe);
    --dump-outputs writes the last timed step's loss and weight samples as float32 .npy files, and
    a second run with the same arguments starts from the same inputs and writes the same values."""
    import numpy as np

    out = _plain_run(tmp_path / "a")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out
    assert out["ms_per_step"] > 0 and out["value"] > 0
    for key in ("fp32_ms_per_step", "speedup_vs_fp32", "fp8", "fp16", "allreduce_probe"):
        assert key not in out
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["loss.npy", "master_weights.npy", "weights.npy"]
    assert all(v.dtype == np.float32 and v.size > 0 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    assert a["loss.npy"].shape == (1,) and abs(float(a["loss.npy"][0]) - out["final_loss"]) <= 1e-4
    assert a["weights.npy"].shape == a["master_weights.npy"].shape
    _plain_run(tmp_path / "b")
    for f, v in a.items():
        np.testing.assert_allclose(np.load(tmp_path / "b" / f), v, rtol=1e-5, atol=1e-6)


def test_extra_passes_run_only_with_full():
    """bench.extra_passes is the one place that decides what runs besides the headline loop (the
    rehearsal never takes the default fp8 pass, so the subprocess tests cannot show that gate)."""
    import argparse

    import bench

    def passes(world=1, rehearsal=False, **kw):
        a = dict(full=False, fp32_only=False, no_fp32=False, fp8=False, no_fp8=False, fp16=False)
        a.update(kw)
        return bench.extra_passes(argparse.Namespace(**a), world, rehearsal)

    none = dict(fp8=False, fp16=False, allreduce_probe=False, fp32=False)
    assert passes() == none and passes(world=8) == none
    assert passes(no_fp8=True, no_fp32=True) == none
    # --full on one GPU: the fp32 pass and the default fp8 pass, each with its own off switch
    assert passes(full=True) == dict(none, fp8=True, fp32=True)
    assert passes(full=True, no_fp8=True) == dict(none, fp32=True)
    assert passes(full=True, no_fp32=True) == dict(none, fp8=True)
    assert passes(full=True, rehearsal=True) == dict(none, fp32=True)
    # N > 1: the probe, fp8 only when asked for; --fp16 anywhere
    assert passes(full=True, world=8) == dict(none, allreduce_probe=True, fp32=True)
    assert passes(full=True, world=8, fp8=True, fp16=True) == dict(fp8=True, fp16=True, allreduce_probe=True, fp32=True)
    # --fp32-only times the fp32 step alone
    assert passes(fp32_only=True) == dict(none, fp32=True)
    assert passes(full=True, fp32_only=True, fp8=True, fp16=True, world=8) == dict(none, fp32=True)


def test_extra_pass_flags_need_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-rehearsal", "--fp16"], cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 2 and "--full" in r.stderr


@pytest.mark.parametrize("n", [2, 4])
def test_bench_n_rank_path_on_gloo(n):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    env.pop("APEX_DDP_MESSAGE_SIZE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", str(n), "--cpu-rehearsal", "--full", "--steps", "2", "--warmup", "1"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout  # rank 0 prints ONE JSON line, nothing else on stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["steps"] == 2 and out["warmup"] == 1
    assert out["config"]["parallelism"] == f"dp{n}" and out["config"]["global_batch"] == 8 * n
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    d = out["dist"]
    assert d["preflight"]["ok"] is True and d["preflight"]["nranks"] == n
    assert d["bucket_choice"].startswith("probe") and len(d["bucket_probe"]) == 3
    assert d["message_size"] in [p["numel"] for p in d["bucket_probe"]]
    assert out["allreduce_probe"]["bytes"] > 0 and out["allreduce_probe"]["us"] > 0
    assert out["ddp"]["world_size"] == n and out["ddp"]["num_buckets"] >= 2
    assert out["fp32_ms_per_step"] > 0 and out["speedup_vs_fp32"] > 0
    assert "rehearsal" in out and "NOT a measurement" in out["rehearsal"]
