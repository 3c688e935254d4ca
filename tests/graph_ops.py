"""TEST-ONLY: a kernel layer that can RECORD, with the semantics that make hipGraph replays go stale, on the CPU oracle.

`DeferringOps(inner)` hands every call through to `inner` (tests/oracle_ops.py: OracleOps) and offers the four graph operations the
ExaSlang-4 interpreter's `auto_graph` needs of a kernel layer (exastencils_amd/ops.py: graph_begin / graph_end / graph_replay /
graph_capturing).  While a recording is open, a kernel-layer call executes nothing: it is put on the recording's list with its
arguments as a hipGraph node keeps them -- numbers, boxes and lists BY VALUE (copied when the call is made), arrays and layout /
stencil / geometry objects BY REFERENCE (a pointer in the node) -- and a replay executes the list.  So a scalar the interpreter took
from a global when it issued the loop is frozen in the recording, and a launch the interpreter decided not to issue is not in it:
what a stream capture does on the device.  Plumbing (allocation, pointers; the set of tools/record_choreography.py) runs at once;
a call that hands a value back to the host while recording raises RuntimeError, as a capture would.  Never imported by the package."""
import ctypes

from oracle_ops import OracleOps

# no launch: runs at once, recording or not (tools/record_choreography.py draws the same line)
PLUMBING = {"new_array", "new_scalar", "ptr", "synchronize", "side_stream", "to_host", "from_host", "scalar_value"}
# these hand a device value to the host (a synchronisation inside a capture), or return one the interpreter goes on to read
TO_HOST = {"to_host", "scalar_value", "dot", "sum", "residual_norm2", "max_err_fn", "max_err_expr", "max_err_expr_cell"}


class PlanesOps(OracleOps):
    """OracleOps with two traits of the HIP layer that a recording can get wrong.  The one entry point the interpreter needs to APPLY `transform coeff with [x, y, z, i] => [i, x, y, z]`: the
    oracle's loops read coefficient planes, so this layer's "transformed" copy is a copy in the same order -- still a second array
    that the loops read and that goes out of date when the planes are rewritten (Exa4Program.stencil, _sf_dirty)."""

    def transform_stencilfield(self, lc, nent, src, dst, to_entry_fastest):
        dst.copy_(src)

    def residual_restrict(self, lu, u, lf, rhs, lr, res, st, lc, fc, scale, fbegin, fend, cbegin, cend):
        """As the one-pass HIP kernel: the residual goes into the restriction and is never stored -- `res` keeps what it held, so a run
        that issues the two loops one by one leaves another (dead) array than a run that issues them as one pass."""
        OracleOps.residual_restrict(self, lu, u, lf, rhs, lr, res.clone(), st, lc, fc, scale, fbegin, fend, cbegin, cend)


def _by_value(v):
    if isinstance(v, (list, tuple, ctypes.Array)):
        return [_by_value(x) for x in v]
    return v        # numbers are values already; tensors, structs, stencils, programs: the node holds a reference


class DeferringOps:
    """Every attribute of `inner`, absent ones included (hasattr answers as for `inner`); see the module's docstring."""

    def __init__(self, inner=None):
        self.__dict__.update(_inner=inner or PlanesOps(), _open=None, recordings=0, replays=0)

    # -- the four graph operations ----------------------------------------------------------------------------------------
    def graph_begin(self):
        if self._open is not None:
            raise RuntimeError("a recording is already open")
        self.__dict__["_open"] = []
        self.__dict__["recordings"] += 1
        return self._open

    def graph_end(self, rec):
        assert rec is self._open
        self.__dict__["_open"] = None

    def graph_replay(self, rec):
        assert self._open is None
        self.__dict__["replays"] += 1
        for name, args, kwargs in rec:
            getattr(self._inner, name)(*args, **kwargs)

    def graph_capturing(self) -> bool:
        return self._open is not None

    # -- everything else ----------------------------------------------------------------------------------------------------
    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr) or name.startswith("_") or isinstance(attr, type) or name == "torch":
            return attr

        def call(*args, **kwargs):
            if self._open is None:
                return attr(*args, **kwargs)
            if name in TO_HOST:
                raise RuntimeError("%s hands a value to the host while a recording is open" % name)
            if name in PLUMBING:
                return attr(*args, **kwargs)
            self._open.append((name, [_by_value(a) for a in args], {k: _by_value(v) for k, v in kwargs.items()}))
            return None
        return call

    def __setattr__(self, name, value):
        setattr(self._inner, name, value)
