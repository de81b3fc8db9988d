"""bench.py output contract: one JSON line on stdout with the BASELINE.json metric and config.

The GPU tests share one short single-GPU bench run in a child process (batch 64, MIOpen solver
search off so no find-db miss can stall it) and check every field the round driver reads and the
arrays ``--dump-outputs`` writes."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config"}


def test_bench_metric_matches_baseline():
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        metric = json.load(f)["metric"]
    with open(os.path.join(ROOT, "bench.py")) as f:
        src = f.read()
    assert json.dumps(metric) in src, "bench.py must report the BASELINE.json metric verbatim"


def test_bench_options():
    """The options every caller may pass are there: ``--full`` (off by default) and ``--dump-outputs``."""
    r = subprocess.run([sys.executable, "bench.py", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--gpus GPUS", "--steps STEPS", "--warmup WARMUP", "--dump-outputs DIR", "[--full]"):
        assert opt in r.stdout, opt


@pytest.fixture(scope="module")
def bench_run(tmp_path_factory):
    dump = tmp_path_factory.mktemp("bench_outputs")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--batch", "64",
                        "--conv-benchmark", "0", "--dump-outputs", str(dump)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=110)
    return r, dump


@pytest.mark.gpu
def test_bench_json_line(bench_run):
    r, _ = bench_run
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert REQUIRED <= set(out)
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1
    assert out["dtype"] == "bf16" and out["scaling"] == "weak" and out["higher_is_better"] is True
    assert out["config"]["model"] == "resnet50" and out["config"]["global_batch"] == 64
    assert out["value"] > 0 and abs(out["value"] - 64 * 2 / (out["ms_per_step"] * 2 / 1000)) / out["value"] < 0.01


@pytest.mark.gpu
def test_bench_dump_outputs(bench_run):
    """``--dump-outputs``: the last step's loss, the (sampled) parameters and the BatchNorm statistics,
    as finite float32 arrays of at most 64 MB in all; the dumped loss is the one the result line reports."""
    import numpy as np

    r, dump = bench_run
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    files = sorted(os.listdir(dump))
    assert files == ["bn_running_stats.npy", "metric_loss.npy", "params.npy"]
    arrays = {f[:-4]: np.load(os.path.join(dump, f)) for f in files}
    assert sum(v.nbytes for v in arrays.values()) <= 64 * 10**6
    for name, v in arrays.items():
        assert v.dtype == np.float32 and v.ndim == 1 and v.size > 0 and np.isfinite(v).all(), name
    assert arrays["metric_loss"].shape == (1,)
    assert abs(float(arrays["metric_loss"][0]) - out["config"]["final_loss"]) <= 1e-4
    # ResNet-50: 25.6M parameters are sampled down, the ~53k BatchNorm statistics are written whole
    assert arrays["params"].size == 4 * 2**20 and arrays["params"].std() > 0
    assert arrays["bn_running_stats"].size == 2 * 26560
