"""bench.py's plain run (the headline line alone, exactly --steps timed LM iterations) and --dump-outputs (the parameters after the
last timed step, the same from run to run and with or without --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "small", "--steps", "5", "--warmup", "2",
                          "--dump-outputs", str(out_dir), *extra], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_and_dumped_outputs(tmp_path):
    d = _bench(tmp_path / "plain")
    assert d["metric"] == "ba_iterations_per_sec" and d["unit"] == "it/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 5 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["ba_cost"]["iterations"] == 7                      # counted from the start of the problem: warm-up + timed steps
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) <= 1e-6 * 1e3
    assert d["ba_cost"]["after_timed_steps"] < d["ba_cost"]["initial"]
    # nothing beyond the headline in a plain run
    for k in ("roofline", "matched_pairs_per_sec", "cpu_baseline", "roofline_gemm", "ba_solve_end_to_end"):
        assert k not in d, k
    a = {n: np.load(tmp_path / "plain" / f"{n}.npy") for n in ("intrinsics", "extrinsics", "points", "ba_cost")}
    assert a["intrinsics"].shape == (4,) and a["extrinsics"].shape == (12, 6) and a["points"].shape == (5000, 3)
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in a.values())
    assert a["ba_cost"][1] == d["ba_cost"]["after_timed_steps"]

    # --full times more after the BA steps, but dumps the same arrays: the inputs are seeded and the reductions deterministic
    f = _bench(tmp_path / "full", "--full", "--no-cpu-baseline", "--no-gemm")
    assert f["steps"] == 5 and f["roofline"] is not None and f["matched_pairs_per_sec"]["value"] > 0
    for n, v in a.items():
        assert np.array_equal(np.load(tmp_path / "full" / f"{n}.npy"), v), n
