"""bench.py end to end on one GPU, tiny shapes: a plain run prints the headline line only (the extra measurements are --full's)
and, with --dump-outputs, writes the last timed step's losses and parameters; --full still adds its measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--gpus", "1", "--batch", "2", "--T", "32", "--D", "64", "--stage", "3"]
FULL_ONLY = ("eager_ms_per_step", "f32", "bf16_features", "other_configs", "trainer", "cpu_baseline")


def run_bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DRN_FORCE_DEVICE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + TINY + args, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-4000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    d = run_bench(["--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path)])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 5 and d["warmup"] == 2 and d["unit"] == "clips/s" and d["higher_is_better"] is True
    assert abs(d["value"] - 2 / (d["ms_per_step"] * 1e-3)) <= 0.01 * d["value"]
    assert not any(k in d for k in FULL_ONLY), sorted(d)
    assert "kernel" not in d["roofline"] and d["roofline"]["path"]["path_frac"] > 0
    names = os.listdir(str(tmp_path))
    assert "loss_cls.npy" in names and "loss_reg.npy" in names and "param.prop_fc.weight.npy" in names
    cls = np.load(str(tmp_path / "loss_cls.npy"))
    assert cls.dtype == np.float32 and np.isfinite(cls).all()
    assert abs(float(cls.reshape(-1)[0]) - d["config"]["loss_cls"]) <= 1e-6 * max(1.0, abs(d["config"]["loss_cls"]))
    assert sum(os.path.getsize(str(tmp_path / n)) for n in names) <= 64 << 20


def test_dump_is_the_same_whichever_graph_is_timed(tmp_path):
    """The warm-up A/B picks the linear or the two-branch hipGraph by wall clock; the model the timed steps train has the same history
    either way, so the dumps of a linear-only and a two-branch-only run must be equal file for file -- which also holds only if both
    dump the model the timed steps updated.  Two runs of the same graph reproduce each other as well."""
    lin = run_bench(["--steps", "4", "--warmup", "2", "--no-forked", "--dump-outputs", str(tmp_path / "linear")])
    fk = run_bench(["--steps", "4", "--warmup", "2", "--force-forked", "--dump-outputs", str(tmp_path / "forked")])
    fk2 = run_bench(["--steps", "4", "--warmup", "2", "--force-forked", "--dump-outputs", str(tmp_path / "forked2")])
    assert "two branches" not in lin["config"]["launch"] and "two branches" in fk["config"]["launch"], (lin["config"], fk["config"])
    assert lin["config"]["loss_cls"] == fk["config"]["loss_cls"] == fk2["config"]["loss_cls"]
    names = sorted(os.listdir(str(tmp_path / "linear")))
    assert names == sorted(os.listdir(str(tmp_path / "forked"))) == sorted(os.listdir(str(tmp_path / "forked2")))
    assert any(n.startswith("param.") for n in names) and any(n.startswith("buffer.") for n in names)
    for n in names:
        a = np.load(str(tmp_path / "linear" / n))
        assert np.array_equal(a, np.load(str(tmp_path / "forked" / n))), n
        assert np.array_equal(a, np.load(str(tmp_path / "forked2" / n))), n


def test_full_run_keeps_the_extra_measurements():
    d = run_bench(["--steps", "3", "--warmup", "1", "--full", "--cpu-steps", "1", "--no-other-configs", "--no-trainer"])
    assert d["steps"] == 3
    for k in ("eager_ms_per_step", "f32", "bf16_features", "cpu_baseline"):
        assert k in d, k
    roof = d["roofline"]                           # (per-kernel timing; TFLOP/s round to 0 at these shapes, the launch times do not)
    assert roof["kernel"] and roof["launches_per_step"] >= 1 and roof["avg_launch_ms_eager"] > 0 and "sustained" in roof
