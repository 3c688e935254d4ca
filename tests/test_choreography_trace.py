"""The host layer issues the same kernel-layer and communicator calls, in the same order, on the same boxes and arrays (and, on the
GPU, each while the same stream was the current one) as the traces under tests/traces/ say -- recorded by tools/record_choreography.py
before the choreography was last rewritten.  The tests of the results compare bits only: a pass issued twice, an exchange too many or a
launch that moved to the other stream passes them.  A change that means to alter the choreography records the traces anew and says so.

Not covered: how the two streams are ordered against each other.  The traces hold which stream was current at each call, not the
fork and join (`wait_stream`) around them; a join that went missing would pass here and is left to the bit-for-bit tests
(test_jacobi_pair_overlap_equals_sequential, test_rbgs_sweep_overlap_equals_sequential)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_choreography", os.path.join(ROOT, "tools", "record_choreography.py"))
rc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rc)

from test_gpu_kernels import hip  # noqa: E402,F401  (fixture)


def _same(got, want):
    assert len(got) == len(want), "%d calls, the recorded trace has %d" % (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert json.dumps(g, sort_keys=True) == json.dumps(w, sort_keys=True), "call %d: %r, the recorded trace has %r" % (i, g, w)


@pytest.mark.parametrize("name", sorted(rc.CPU))
def test_cpu_choreography(name):
    want = rc.load(rc.path_of("cpu"))[name]
    assert want, "an empty trace checks nothing"
    _same(rc.plain(rc.record_cpu(name)), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(rc.GPU))
def test_gpu_choreography(hip, name):  # noqa: F811
    want = rc.load(rc.path_of("gpu"))[name]
    assert any(ev.get("side") for ev in want), "the recorded trace must hold the side-stream branch"
    _same(rc.plain(rc.record_gpu(name, hip)), want)
