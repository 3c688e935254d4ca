"""bench.py as it is run for every change: a plain run prints the headline line and nothing of --full, and --dump-outputs writes
what the timed steps computed -- the same arrays for the same arguments, and the same bits as K single steps (one launch each),
so that --steps K is the number of steps taken at every size: 256^3 runs passes of three steps, 64^3 has no three-step pass."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "2", "--settle-steps", "4"] + args,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.parametrize("level", [8, 6])
def test_plain_run_and_its_dumped_outputs(level, tmp_path):
    runs = {}
    for name, steps, extra in (("a", 7, []), ("b", 7, []), ("single", 7, ["--no-temporal-blocking"]), ("longer", 8, [])):
        r = _bench(["--level", str(level), "--steps", str(steps), "--dump-outputs", str(tmp_path / name)] + extra)
        assert r["metric"] == "LU/s" and r["unit"] == "LU/s" and r["higher_is_better"] is True and r["dtype"] == "f64"
        assert r["steps"] == steps and r["value"] > 0 and r["ms_per_step"] > 0
        assert not {"roofline", "sustained_value", "vcycle_ms", "roofline_kernels", "cpu_baseline"} & set(r), sorted(r)
        runs[name] = {f: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))}
    assert sorted(runs["a"]) == ["solution_midplane.npy", "solution_sample.npy"]
    for f, x in runs["a"].items():
        assert x.dtype == np.float64 and np.isfinite(x).all()
        assert np.array_equal(x, runs["b"][f]) and np.array_equal(x, runs["single"][f]), f
    assert not np.array_equal(runs["a"]["solution_sample.npy"], runs["longer"]["solution_sample.npy"])
