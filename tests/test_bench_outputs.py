"""bench.py without --full times the headline only, and --dump-outputs writes what its last timed step computed.

CPU: the argument surface and the dump writer (float32, the 64 MB cap as a fixed sample).
GPU (-m gpu): two plain runs with the same arguments print the headline line without the --full blocks and dump identical arrays.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("config1", "alt", "encode_only_dense", "hbm_copy_measured_GBs", "inference_ms_per_frame", "dataset", "config4",
             "cpu_baseline", "train_step", "build_stamp")


def test_full_and_dump_outputs_are_options():
    import bench
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "out_dir"])
    assert a.full is True and a.dump_outputs == "out_dir"


def test_dump_outputs_writes_float32_whole_or_a_fixed_sample(tmp_path):
    import bench
    rng = np.random.RandomState(0)
    frame = rng.rand(4, 16, 16)                                           # float64 in, float32 out
    feats = rng.rand(4, 64, 8).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "whole"), {"frame": frame, "features": feats})
    f = np.load(tmp_path / "whole" / "frame.npy")
    assert f.dtype == np.float32 and f.shape == frame.shape and np.array_equal(f, frame.astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "whole" / "features.npy"), feats)
    # over the budget every array keeps its share as the same seeded flat sample, run after run
    budget = (frame.size + feats.size) * 4 // 4                           # a quarter of the float32 bytes
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"frame": frame, "features": feats}, budget=budget)
    sizes = 0
    for name, src in (("frame", frame), ("features", feats)):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and a.ndim == 1 and np.array_equal(a, b)
        assert np.isin(a, src.astype(np.float32).reshape(-1)).all()
        sizes += a.nbytes
    assert 0 < sizes <= budget


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--grid", "128", "--batch", "4",
                        "--jacobi", "20", "--dump-outputs", str(out_dir)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[:600]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_repeatable_outputs(tmp_path):
    d = _plain_run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert abs(d["value"] - 4 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    assert not [k for k in FULL_ONLY if k in d], [k for k in FULL_ONLY if k in d]
    assert d["leg_order"] == ["headline"]
    assert d["effective_warmup_steps"]["headline_preroll"] == 2 * (1 + 3)   # the headline step in place of configs[1] and alt
    frame, feats = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "a" / "features.npy")
    assert frame.dtype == feats.dtype == np.float32
    assert frame.shape == (4, 128, 128) and feats.shape == (4, 1024, 128)
    assert np.isfinite(frame).all() and np.isfinite(feats).all() and frame.max() > 0
    _plain_run(tmp_path / "b")
    for name in ("frame", "features"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")), name
