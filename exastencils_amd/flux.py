"""What one explicit flux-form update is (include/examg.h: examg_flux_t), Python side: the programs, and per component the constant
axis stencil on one input field and the scaled differences of a program at two cells.  The kernel layers take a FluxSpec with the
arrays of a call; FluxSpec.c_struct binds them."""
from __future__ import annotations

from dataclasses import dataclass, field as _dcf
from typing import List, Sequence, Tuple

from . import lib as _lib

ZERO = (0, 0, 0)


@dataclass(frozen=True)
class FluxTerm:
    """scale * (P(i + plus) - P(i + minus)), P the program `prog` of the spec."""
    prog: int
    plus: Tuple[int, int, int]
    minus: Tuple[int, int, int]
    scale: float


@dataclass(frozen=True)
class FluxComp:
    """out = fold of the entries (offsets, coefs) over the input field `field`, then + every term in declared order."""
    field: int
    offsets: Tuple[Tuple[int, int, int], ...]
    coefs: Tuple[float, ...]
    terms: Tuple[FluxTerm, ...] = ()


@dataclass
class FluxSpec:
    """programs: lists of (opcode name, constant or None) over lib.FLUX_OPS (`f<k>`: input field k at the cell)."""
    programs: List[list] = _dcf(default_factory=list)
    comps: List[FluxComp] = _dcf(default_factory=list)

    def c_struct(self, ptr_of, lin, ins: Sequence, lout, outs: Sequence) -> "_lib.FluxC":
        """The call's examg_flux_t.  Counts over the library's limits still reach the library (it names the refusal); what would not fit
        the arrays of the struct is cut off behind the limit."""
        import ctypes as C

        fx = _lib.FluxC()
        fx.nfields, fx.nprogs, fx.ncomp = len(ins), len(self.programs), len(self.comps)
        C.memmove(C.byref(fx.lin), C.byref(lin), C.sizeof(_lib.LayoutC))
        C.memmove(C.byref(fx.lout), C.byref(lout), C.sizeof(_lib.LayoutC))
        for k, x in enumerate(ins[:_lib.FLUX_MAX_FIELDS]):
            fx.in_[k] = ptr_of(x)
        for c, x in enumerate(outs[:_lib.FLUX_MAX_COMP]):
            fx.out[c] = ptr_of(x)
        for p, prog in enumerate(self.programs[:_lib.FLUX_MAX_PROGS]):
            e = prog if isinstance(prog, _lib.NlExprC) else _flux_program(prog)
            C.memmove(C.byref(fx.prog[p]), C.byref(e), C.sizeof(_lib.NlExprC))
        for c, comp in enumerate(self.comps[:_lib.FLUX_MAX_COMP]):
            cc = fx.comp[c]
            cc.field, cc.nent, cc.nterms = comp.field, len(comp.offsets), len(comp.terms)
            for k, (o, v) in enumerate(list(zip(comp.offsets, comp.coefs))[:_lib.FLUX_MAX_ENTRIES]):
                for d in range(3):
                    cc.off[k][d] = o[d]
                cc.coef[k] = float(v)
            for m, t in enumerate(comp.terms[:_lib.FLUX_MAX_TERMS]):
                tm = cc.term[m]
                tm.prog, tm.scale = t.prog, float(t.scale)
                for d in range(3):
                    tm.plus[d], tm.minus[d] = t.plus[d], t.minus[d]
        return fx


def _flux_program(prog) -> "_lib.NlExprC":
    """The program as the library takes it.  What the binding's table does not know (a refused opcode under test: ("op", code)) and
    programs over the length limit travel as they are: the library names the refusal."""
    e = _lib.NlExprC()
    e.n = len(prog)
    for i, (name, c) in enumerate(prog[:_lib.MAX_NL_EXPR]):
        e.op[i] = int(c) if name == "op" else _lib.FLUX_OPS[name]
        e.c[i] = float(c) if c is not None and name != "op" else 0.0
    e.program = list(prog)
    return e


def field_program(prog) -> "_lib.NlExprC":
    """examg_nlexpr_t of a program over several cell fields (examg_reduce_expr_cell)."""
    return _flux_program(prog)
