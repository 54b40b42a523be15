"""bench.py: a plain run measures the headline figure and nothing else; --full adds the side measurements (residual,
roofline with the MFMA probe and the live HBM traffic, the un-bracketed step, the task-API leg, the CPU baseline).
The CPU tests drive main() around a canned run_single; the GPU test runs both commands on a small workload."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
SIDE = ("roofline", "unprofiled_ms", "worker_path", "cpu_baseline", "residual")


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_modes_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _main(bench, monkeypatch, capsys, argv):
    """main() with the GPU part canned: 2 steps of 0.5 s each at N=3000; what run_single saw and which legs ran."""
    seen, legs = {}, []

    def run_single(a):
        seen["full"] = a.full
        r = {"elapsed": 1.0, "upd_ms": 800.0, "upd_flops": 8e12, "upd_launches": 10, "regimes": {"waves": 3},
             "residual": None, "probe": None, "kernel": "k_trail_update", "calibration": [70.0, 40.0, 140.0, 30.0] + [0.0] * 4,
             "counters": True, "unprofiled_ms": None, "dump": None}
        if a.full:
            r.update(probe=75.0, unprofiled_ms=499.0, residual=None if a.no_check else 1e-16)
        return r

    monkeypatch.setattr(bench, "run_single", run_single)
    monkeypatch.setattr(bench, "live_pmc_traffic", lambda a: legs.append("traffic") or (1e9, 10, "measured in this run"))
    monkeypatch.setattr(bench, "worker_path", lambda N, B: legs.append("worker") or {"N": N, "tile": B})
    monkeypatch.setattr(bench, "cpu_baseline", lambda N, B, seed, vendor=True: legs.append("cpu") or {"value": 1.0})
    monkeypatch.setattr(sys, "argv", ["bench.py", "--N", "3000", "--steps", "2", "--warmup", "0"] + argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert bench.main() == 0
    out = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(out) == 1, out
    return json.loads(out[0]), seen, legs


def test_full_is_off_by_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full"])
    assert bench.parse().full is True


def test_plain_run_prints_the_headline_and_runs_no_side_leg(bench, monkeypatch, capsys):
    line, seen, legs = _main(bench, monkeypatch, capsys, [])
    assert seen == {"full": False} and legs == []
    assert all(k in line for k in HEADLINE) and not any(k in line for k in SIDE)
    # 2 steps in 1.0 s: 500 ms per step, N^3/3 flops each
    assert line["ms_per_step"] == 500.0 and line["value"] == round(3000 ** 3 / 3.0 * 2 / 1.0 / 1e12, 3)
    assert line["unit"] == "TFLOP/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["metric"].startswith("fp64 TFLOP/s for NxN SPD Cholesky")
    # the schedule the figure was measured on costs nothing to record and stays
    assert line["config"]["schedule_regimes"] == {"waves": 3} and line["config"]["schedule_calibration"]["device_counters"] is True


def test_the_no_switches_change_nothing_in_a_plain_run(bench, monkeypatch, capsys):
    plain, _, _ = _main(bench, monkeypatch, capsys, [])
    line, _, legs = _main(bench, monkeypatch, capsys, ["--no-cpu-baseline", "--no-worker-path", "--no-live-traffic", "--no-check"])
    assert legs == [] and line == plain


def test_full_run_adds_every_side_leg_to_the_same_headline(bench, monkeypatch, capsys):
    plain, _, _ = _main(bench, monkeypatch, capsys, [])
    line, seen, legs = _main(bench, monkeypatch, capsys, ["--full"])
    assert seen == {"full": True} and legs == ["traffic", "worker", "cpu", "cpu"]  # (the CPU baseline has a second size)
    assert all(k in line for k in SIDE)
    assert {k: line[k] for k in HEADLINE} == {k: plain[k] for k in HEADLINE}
    assert line["roofline"]["achieved"] == 10.0 and line["roofline"]["peak_probe"] == 75.0 and line["roofline"]["traffic"] == 1e9
    assert line["unprofiled_ms"] == 499.0 and line["residual"] == 1e-16
    # a leg switched off leaves a --full run as before
    line, _, legs = _main(bench, monkeypatch, capsys, ["--full", "--no-cpu-baseline", "--no-worker-path", "--no-live-traffic", "--no-check"])
    assert legs == [] and "roofline" in line and "unprofiled_ms" in line
    assert not any(k in line for k in ("worker_path", "cpu_baseline", "residual"))


@pytest.mark.gpu
def test_plain_and_full_runs_on_a_small_workload():
    """Both commands for real at N=2048, tile 512 (four tile columns: every kernel of the schedule runs): the plain line
    carries no side measurement, the --full line carries them all, and both dump the same factor (to rounding)."""
    import numpy as np
    import tempfile

    def run(extra, out_dir):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--N", "2048", "--tile", "512", "--steps", "1",
                            "--warmup", "1", "--dump-outputs", out_dir] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, p.stdout
        return json.loads(lines[0])

    with tempfile.TemporaryDirectory() as tmp:
        plain = run([], os.path.join(tmp, "plain"))
        full = run(["--full", "--no-live-traffic", "--cpu-N", "2048", "--cpu-extra-N", "0", "--worker-path-N", "2048"],
                   os.path.join(tmp, "full"))
        assert all(k in plain for k in HEADLINE) and not any(k in plain for k in SIDE)
        assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["outputs"]["arrays"] == full["outputs"]["arrays"]
        assert all(k in full for k in SIDE), sorted(full)
        # fp64 factor of a matrix with N on its diagonal: the residual is a few ulps (the suite's bound for this path)
        assert full["residual"] <= 1e-13 and "error" not in full["worker_path"]
        for name in plain["outputs"]["arrays"]:
            a, b = np.load(os.path.join(tmp, "plain", name + ".npy")), np.load(os.path.join(tmp, "full", name + ".npy"))
            # two processes calibrate twice and may run two schedules, which round differently: n * eps * O(1) for this
            # well-conditioned matrix, 2048 * 1.1e-16 = 2.3e-13 (the sampled indices are exact)
            assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), name
