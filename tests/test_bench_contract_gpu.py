"""GPU: `python bench.py` keeps the driver's contract - exactly one JSON line on stdout with the fields the driver and
the judge read (metric / value / unit / n_gpus / steps / warmup / ms_per_step / higher_is_better / scaling /
vs_baseline / dtype / data / config.workload; with --full also `roofline`, `parity` and the extras such as
`cpu_baseline`), and `--dump-outputs` writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_fields():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full", "--no-e2e",
                          "--no-streams", "--no-cpu-baseline"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and "workload" in d["config"]
    assert "model" not in d["config"]
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert d["value"] > 1e4 and abs(d["ms_per_step"] * d["value"] / 1e3 - 256) < 1.0      # value = batch / step time
    assert d["parity"]["max_abs_logit_err_vs_oracle"] <= 1e-3


def test_two_rank_launch_of_the_bench_rehearsed_on_one_gpu():
    """The driver starts `--gpus N` as `python -m torch.distributed.run ... bench.py --gpus N`.  With DFD_BENCH_REHEARSE=1
    two ranks share this box's GPU (torch.distributed over gloo, vote exchange on the documented torch fallback): the
    multi-rank control flow of the file - barriers, MAX-over-ranks timing, aggregate value, the frame-sharded streams
    with every frame verified against the single-GPU sequence - runs on real hardware before an 8-GPU node ever sees it.
    A rehearsal of control flow, not a measurement."""
    env = dict(os.environ, DFD_BENCH_REHEARSE="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3",
                          "--warmup", "1", "--full", "--no-e2e", "--no-cpu-baseline"], cwd=ROOT, capture_output=True, text=True,
                         timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    assert abs(d["ms_per_step"] * d["value"] / 1e3 - 2 * 256) < 2.0                        # whole-job aggregate over both ranks
    c5 = d["config5"]
    assert c5["transport"] == "torch" and c5["verdicts_equal_single_gpu"] is True and c5["verified_frames_per_stream"] == 32 * 2      # every frame of every stream (32 waves x 2 ranks)


def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(tmp_path, pkg, seeded_sd):
    """A plain run (no --full) times the K steps and prints the headline fields and nothing measured beside them;
    --dump-outputs DIR holds the last timed step's logits, which agree with the CPU oracle on bench.py's seeded crops."""
    import torch

    from oracle import b0_ref

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "crops/s" and d["dtype"] == "f32" and "workload" in d["config"]
    assert abs(d["ms_per_step"] * d["value"] / 1e3 - 256) < 1.0
    for key in ("roofline", "parity", "cpu_baseline", "e2e", "config5", "bf16"):
        assert key not in d, key
    y = np.load(tmp_path / "logits.npy")
    assert y.dtype == np.float32 and y.shape == (256, 1) and np.all(np.isfinite(y))
    x = torch.randn(256, 3, 224, 224, generator=torch.Generator().manual_seed(1))[:8]
    want = b0_ref.forward(pkg.weights.to_torch(seeded_sd), x).numpy()
    assert float(np.abs(y[:8] - want).max()) <= 1e-3
