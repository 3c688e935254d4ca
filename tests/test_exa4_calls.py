"""The ExaSlang-4 interpreter issues the same kernel-layer calls, in the same order, on the same boxes and arrays as the traces under
tests/traces/ say (exa4_cpu.json, exa4_gpu.json) -- recorded by tools/record_exa4_calls.py before loop statements were given one
recogniser and one launcher.  The interpreter tests compare printed values and `launches` totals: a pass issued twice, or a loop launched
once where it stands and once more when a pending loop is flushed, passes them.  A change that means to alter the call sequence records
the traces anew and says so.

Beside the calls every scenario pins `launches`, `fusions` and `printed_values`, and that `launches` counts exactly the calls that were
issued.  Not so in the auto_graph scenario, by construction: a replay adds the launches of the recording and logs one graph_replay."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_exa4_calls", os.path.join(ROOT, "tools", "record_exa4_calls.py"))
rx = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rx)

from test_gpu_kernels import hip  # noqa: E402,F401  (fixture)


def _same(got, want):
    assert len(got) == len(want), "%d calls, the recorded trace has %d" % (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert json.dumps(g, sort_keys=True) == json.dumps(w, sort_keys=True), "call %d: %r, the recorded trace has %r" % (i, g, w)


@pytest.mark.parametrize("name", sorted(rx.CPU))
def test_cpu_exa4_calls(name):
    want, rest = rx.load(rx.path_of("cpu"))[name]
    assert want, "an empty trace checks nothing"
    got, now = rx.record(name)
    _same(got, want)
    assert now["launches"] == rest["launches"] and now["fusions"] == rest["fusions"]
    assert now["printed_values"] == rest["printed_values"]
    if "auto_graph" in name:
        assert any(ev["c"] == "ops.graph_replay" for ev in got), "the trace must hold the recording path"
    else:
        assert rx.launches_logged(got) == now["launches"], "`launches` must count the calls that were issued"


def test_cpu_trace_file_stays_small():
    assert os.path.getsize(rx.path_of("cpu")) < 200 * 1024


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(rx.GPU))
def test_gpu_exa4_calls(hip, name):  # noqa: F811
    """The calls and `launches` of the HIP kernel layer's routes; what the program prints follows the CPU run of the same scenario within
    1e-10 relative (whole solves; when the traces were recorded the largest deviation was 6.1e-11, of the last
    residual norm of poisson3d_rbgs_plain, and 2.0e-16 in the Jacobi and Helmholtz programs)."""
    want, rest = rx.load(rx.path_of("gpu"))[name]
    assert want, "an empty trace checks nothing"
    got, now = rx.record(name, hip)
    _same(got, want)
    assert now["launches"] == rest["launches"] and now["fusions"] == rest["fusions"]
    cpu = rx.load(rx.path_of("cpu"))[name][1]["printed_values"]
    print(name, "gpu", now["printed_values"], "cpu", cpu)
    assert len(now["printed_values"]) == len(cpu) > 0
    for x, y in zip(now["printed_values"], cpu):
        assert abs(x - y) <= 1e-10 * abs(y), (now["printed_values"], cpu)
