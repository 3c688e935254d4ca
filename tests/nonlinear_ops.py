"""TEST-ONLY restatement of the semilinear entry points (include/examg.h: examg_nl_op, examg_nl_smooth) in numpy, on top of the
oracle-backed kernel layer (tests/oracle_ops.py through tests/system_ops.py, so that one class runs every program of the suite).
Every operation in the order the header fixes: the stencil's entries folded left to right in declared order, then c(q) * u added,
the programs evaluated instruction by instruction.  numpy evaluates each operation in IEEE double, one at a time: no contraction."""
import numpy as np

from cell_ops import _empty, _sl, _view
from system_ops import SystemOracleOps, _fold

NL_APPLY, NL_RESIDUAL, NL_ADD = 0, 1, 2
MAX_NL_EXPR, NL_STACK = 32, 8

_UN = {"neg": np.negative, "sin": np.sin, "cos": np.cos, "exp": np.exp, "sinh": np.sinh, "cosh": np.cosh, "sqrt": np.sqrt, "tan": np.tan,
       "log": np.log, "fabs": np.abs, "tanh": np.tanh}
_BI = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide, "pow": np.power, "max": np.maximum, "min": np.minimum}


def check_program(prog):
    """The header's conditions on a program: what the library refuses raises here."""
    if not 1 <= len(prog) <= MAX_NL_EXPR:
        raise ValueError("point program with %d instructions (limit %d)" % (len(prog), MAX_NL_EXPR))
    sp = 0
    for name, _ in prog:
        if name in ("const", "u"):
            sp += 1
        elif name in _BI:
            if sp < 2:
                raise ValueError("point program underflows its stack")
            sp -= 1
        elif name in _UN:
            if sp < 1:
                raise ValueError("point program underflows its stack")
        else:
            raise ValueError("point program with the instruction %r" % name)
        if sp > NL_STACK:
            raise ValueError("point program needs a stack deeper than %d" % NL_STACK)
    if sp != 1:
        raise ValueError("point program must leave exactly one value")


def eval_program(prog, v):
    """The program on the array of field values v, one IEEE operation per instruction."""
    st = []
    for name, c in prog:
        if name == "const":
            st.append(np.full(v.shape, float(c)))
        elif name == "u":
            st.append(v)
        elif name in _UN:
            st[-1] = _UN[name](st[-1])
        else:
            b = st.pop()
            st[-1] = _BI[name](st[-1], b)
    return st[0]


def _program(c):
    prog = c.program if hasattr(c, "program") else list(c)
    check_program(prog)
    return prog


def _colour_sel(begin, end, colour):
    i2, i1, i0 = np.meshgrid(np.arange(begin[2], end[2]), np.arange(begin[1], end[1]), np.arange(begin[0], end[0]), indexing="ij")
    return ((i0 + i1 + i2) % 2) == colour


class NonlinearOracleOps(SystemOracleOps):
    name = "nonlinear-oracle"

    @staticmethod
    def _n(lu, u, lq, q, st, c, begin, end):
        """N = conv(A, u) + (c(q) * u) on the box."""
        if st.cfield is not None:
            raise ValueError("a stencil field cannot be the constant stencil of a semilinear operator")
        ua, uref = _view(lu, u)
        qa, qref = _view(lq, q)
        conv = _fold(st, ua, uref, begin, end, False)
        with np.errstate(all="ignore"):
            cv = eval_program(_program(c), qa[_sl(qref, begin, end)])
            return conv + cv * ua[_sl(uref, begin, end)]

    def nl_op(self, mode, lu, u, lq, q, lf, rhs, ld, dst, st, c, begin, end):
        if _empty(begin, end):
            return
        n = self._n(lu, u, lq, q, st, c, begin, end)
        da, dref = _view(ld, dst)
        s = _sl(dref, begin, end)
        if mode == NL_APPLY:
            da[s] = n
        elif mode == NL_RESIDUAL:
            fa, fref = _view(lf, rhs)
            da[s] = fa[_sl(fref, begin, end)] - n
        elif mode == NL_ADD:
            da[s] = da[s] + n
        else:
            raise ValueError("nl_op: bad mode %r" % (mode,))

    def nl_smooth(self, lu, u_in, ld, u_out, lf, rhs, st, c, d, w, colour, begin, end):
        if _empty(begin, end):
            return
        in_place = u_out.data_ptr() == u_in.data_ptr()
        if colour < 0 and in_place:
            raise ValueError("nl_smooth: colour -1 (Jacobi) runs out of place")
        if colour >= 0 and not in_place:
            raise ValueError("nl_smooth: a colour runs in place")
        if colour >= 0 and any(sum(o) % 2 == 0 for k, o in enumerate(st.offsets) if k != st.diag_index):
            raise ValueError("nl_smooth: the parity colouring does not decouple the stencil")
        n = self._n(lu, u_in, lu, u_in, st, c, begin, end)
        ua, uref = _view(lu, u_in)
        uc = ua[_sl(uref, begin, end)]
        fa, fref = _view(lf, rhs)
        with np.errstate(all="ignore"):          # points of the other colour are computed and thrown away
            dv = eval_program(_program(d), uc)
            new = uc + float(w) * ((fa[_sl(fref, begin, end)] - n) / (float(st.coefs[st.diag_index]) + dv))
        da, dref = _view(ld, u_out)
        s = _sl(dref, begin, end)
        da[s] = new if colour < 0 else np.where(_colour_sel(begin, end, colour), new, da[s])
