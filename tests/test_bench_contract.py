"""Driver-contract test: `python bench.py` emits ONE JSON line from rank 0
with the exact field set and semantics the harness depends on."""

import json
import os
import subprocess
import sys

import numpy as np
import torch

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TINY = ["--batch-size", "2", "--arch", "vit_small", "--local-crops", "2",
        "--global-size", "64", "--local-size", "32"]


def _run_bench(*extra):
    r = subprocess.run(
        [sys.executable, os.path.join(REPO_ROOT, "bench.py"), *extra, *TINY],
        cwd=REPO_ROOT, capture_output=True, text=True, timeout=900,
    )
    assert r.returncode == 0, r.stderr[-800:]
    json_lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(json_lines) == 1, f"expected exactly one JSON line, got {json_lines}"
    return json.loads(json_lines[0])


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's results as float32 .npy
    files, identical from run to run (seeded inputs and weights); --full is
    accepted and leaves the result line's meaning unchanged."""
    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        out = _run_bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(d), *extra)
        assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
        files = sorted(p.name for p in d.iterdir())
        assert {"loss.npy", "total_loss.npy", "student_params_sample.npy",
                "teacher_params_sample.npy"} <= set(files), files
        dumps.append({f: np.load(d / f) for f in files})
    a, b = dumps
    assert a.keys() == b.keys()
    total = 0
    for f, arr in a.items():
        assert arr.dtype == np.float32, (f, arr.dtype)
        assert np.isfinite(arr).all(), f
        total += arr.nbytes
        assert arr.shape == b[f].shape, f
        if not torch.cuda.is_available():
            # fp32 on CPU is bit-reproducible
            np.testing.assert_array_equal(arr, b[f], err_msg=f)
    # on the GPU the same inputs go through bf16 kernels whose reductions use
    # atomics: allow 8 bf16 ulps (2^-8 each) on the loss
    np.testing.assert_allclose(a["loss.npy"], b["loss.npy"], rtol=2.0**-5)
    assert total <= 64 * 2**20
    assert a["student_params_sample.npy"].size > 1000
    # the dumped loss is the step's own return value
    assert a["loss.npy"] == a["total_loss.npy"]


def test_bench_json_contract():
    out = _run_bench("--steps", "1", "--warmup", "0")
    for key, typ in [("metric", str), ("value", float), ("unit", str),
                     ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", float), ("higher_is_better", bool),
                     ("scaling", str), ("dtype", str), ("data", str),
                     ("config", dict)]:
        assert key in out, f"missing {key}"
        assert isinstance(out[key], typ), f"{key}: {type(out[key])}"
    assert out["metric"].startswith("images/sec")
    assert out["higher_is_better"] is True
    assert out["scaling"] == "weak"
    assert out["data"] == "synthetic"
    assert out["n_gpus"] == 1 and out["steps"] == 1 and out["warmup"] == 0
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["vs_baseline"] is None or out["vs_baseline"] > 0
    assert {"model", "global_batch", "parallelism"} <= set(out["config"])
    # whole-job value consistency: value == global_batch * steps / elapsed
    expect = out["config"]["global_batch"] * 1000.0 / out["ms_per_step"]
    assert abs(out["value"] - expect) / expect < 1e-6
