"""TEST-ONLY restatement of the flux-form entry points (include/examg.h: examg_flux_step, examg_reduce_expr_cell, the EXAMG_BC_NEGATE
kind of examg_apply_bc_cell) in numpy, on top of the cell restatement (tests/cell_ops.py).  Every operation in the order the header
fixes: the stencil's entries folded left to right in declared order, then every term in declared order as scale * (P(plus) - P(minus)),
the programs evaluated instruction by instruction on the field values of the one cell they are evaluated at.  numpy evaluates each
operation in IEEE double, one at a time: no contraction.  What the library refuses raises ValueError here."""
import numpy as np

from cell_ops import CellOracleOps, _empty, _sl, _view

FLUX_MAX_FIELDS, FLUX_MAX_PROGS, FLUX_MAX_COMP, FLUX_MAX_TERMS, FLUX_MAX_ENTRIES = 6, 8, 4, 4, 5
MAX_NL_EXPR, NL_STACK = 32, 8
FLUX_GATHER, FLUX_MARCH = 1, 2
REDUCE_MAX, REDUCE_MIN = 0, 1
BC_NEGATE = 2

_UN = {"neg": np.negative, "sin": np.sin, "cos": np.cos, "exp": np.exp, "sinh": np.sinh, "cosh": np.cosh, "sqrt": np.sqrt, "tan": np.tan,
       "log": np.log, "fabs": np.abs, "tanh": np.tanh}
_BI = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide, "pow": np.power, "max": np.maximum, "min": np.minimum}
_AXIS = {(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0)}


def _prog_list(prog):
    return prog.program if hasattr(prog, "program") else list(prog)


def check_program(prog, nfields, what="program"):
    """The header's conditions on a program over cell fields."""
    if len(prog) < 1:
        raise ValueError("%s is empty" % what)
    if len(prog) > MAX_NL_EXPR:
        raise ValueError("%s has %d instructions (limit %d)" % (what, len(prog), MAX_NL_EXPR))
    sp = 0
    for name, _ in prog:
        if name == "const":
            sp += 1
        elif len(name) == 2 and name[0] == "f" and name[1].isdigit() and int(name[1]) < FLUX_MAX_FIELDS:
            if int(name[1]) >= nfields:
                raise ValueError("%s reads field %s; there are %d fields" % (what, name[1], nfields))
            sp += 1
        elif name in _BI:
            if sp < 2:
                raise ValueError("%s underflows its stack" % what)
            sp -= 1
        elif name in _UN:
            if sp < 1:
                raise ValueError("%s underflows its stack" % what)
        else:
            raise ValueError("%s holds the refused instruction %r" % (what, name))
        if sp > NL_STACK:
            raise ValueError("%s needs a stack deeper than %d" % (what, NL_STACK))
    if sp != 1:
        raise ValueError("%s must leave exactly one value" % what)


def eval_program(prog, vals):
    """The program on the arrays vals[k] of the fields' values, one IEEE operation per instruction."""
    st = []
    for name, c in prog:
        if name == "const":
            st.append(np.full(vals[0].shape, float(c)))
        elif name[0] == "f" and name[1:].isdigit():
            st.append(vals[int(name[1:])])
        elif name in _UN:
            st[-1] = _UN[name](st[-1])
        else:
            b = st.pop()
            st[-1] = _BI[name](st[-1], b)
    return st[0]


def _shift(b, e, off):
    return [b[d] + off[d] for d in range(3)], [e[d] + off[d] for d in range(3)]


def _inside(l, b, e, halo):
    for d in range(l.nd):
        ref = l.pad_l[d] + l.ghost_l[d]
        tot = l.pad_l[d] + l.ghost_l[d] + l.dup_l[d] + l.inner[d] + l.dup_r[d] + l.ghost_r[d] + l.pad_r[d]
        if b[d] - halo + ref < 0 or e[d] + halo + ref > tot:
            return False
    return True


def _cell_layout(l, what):
    if any(l.dup_l[d] or l.dup_r[d] for d in range(3)):
        raise ValueError("the %s layout has duplicate layers (a node layout)" % what)
    if l.transform:
        raise ValueError("the %s layout is colour-split" % what)


def check_flux(lin, ins, lout, outs, spec, begin, end):
    """Everything examg_flux_step refuses; True: the box is empty (a no-op)."""
    if lin.nd != 2 or lout.nd != 2:
        raise ValueError("the 3-D kernels are not built")
    _cell_layout(lin, "input")
    _cell_layout(lout, "output")
    if not 1 <= len(ins) <= FLUX_MAX_FIELDS:
        raise ValueError("%d input fields" % len(ins))
    if len(spec.programs) > FLUX_MAX_PROGS:
        raise ValueError("%d programs" % len(spec.programs))
    if not 1 <= len(spec.comps) <= FLUX_MAX_COMP or len(outs) != len(spec.comps):
        raise ValueError("%d components" % len(spec.comps))
    for c, comp in enumerate(spec.comps):
        if any(outs[c].data_ptr() == x.data_ptr() for x in ins):
            raise ValueError("the destination of component %d overlaps an input field" % c)
        if any(outs[c].data_ptr() == outs[k].data_ptr() for k in range(c)):
            raise ValueError("two components write one array")
        if not 0 <= comp.field < len(ins):
            raise ValueError("component %d names field %d" % (c, comp.field))
        if len(comp.offsets) == 0:
            raise ValueError("the stencil of component %d is empty" % c)
        if len(comp.offsets) > FLUX_MAX_ENTRIES or len(comp.terms) > FLUX_MAX_TERMS:
            raise ValueError("component %d: too many entries or terms" % c)
        if any(tuple(o) not in _AXIS for o in comp.offsets):
            raise ValueError("a stencil entry of component %d is not the centre or a unit axis offset" % c)
        for t in comp.terms:
            if not 0 <= t.prog < len(spec.programs):
                raise ValueError("a term of component %d names program %d" % (c, t.prog))
            if tuple(t.plus) not in _AXIS or tuple(t.minus) not in _AXIS:
                raise ValueError("a term of component %d reads a cell off the axes" % c)
    for p, prog in enumerate(spec.programs):
        check_program(_prog_list(prog), len(ins), "program %d" % p)
    if _empty(begin, end):
        return True
    if begin[2] != 0 or end[2] != 1:
        raise ValueError("2-D box must have [0,1) in dim 2")
    if not _inside(lout, begin, end, 0):
        raise ValueError("box leaves the output allocation")
    if not _inside(lin, begin, end, 1):
        raise ValueError("box grown by one cell leaves the input allocation")
    return False


class FluxOracleOps(CellOracleOps):
    name = "flux-oracle"

    def flux_step(self, lin, ins, lout, outs, spec, begin, end):
        if check_flux(lin, ins, lout, outs, spec, begin, end):
            return
        views = [_view(lin, x) for x in ins]
        ref = views[0][1]
        progs = [_prog_list(p) for p in spec.programs]
        cache = {}

        def P(p, off):      # the program at the cells of the box displaced by off: over the values of every field at THAT cell
            key = (p, tuple(off))
            if key not in cache:
                b, e = _shift(begin, end, off)
                with np.errstate(all="ignore"):
                    cache[key] = eval_program(progs[p], [a[_sl(ref, b, e)] for a, _ in views])
            return cache[key]

        results = []
        for comp in spec.comps:
            qa = views[comp.field][0]
            acc = None
            for off, c in zip(comp.offsets, comp.coefs):
                b, e = _shift(begin, end, off)
                t = float(c) * qa[_sl(ref, b, e)]
                acc = t if acc is None else acc + t
            for t in comp.terms:
                with np.errstate(all="ignore"):
                    acc = acc + float(t.scale) * (P(t.prog, t.plus) - P(t.prog, t.minus))
            results.append(acc)
        for out, acc in zip(outs, results):
            da, dref = _view(lout, out)
            da[_sl(dref, begin, end)] = acc

    def flux_route(self, lin, ins, lout, outs, spec, begin, end):
        try:
            return 0 if check_flux(lin, ins, lout, outs, spec, begin, end) else FLUX_MARCH
        except ValueError:
            return -1

    def reduce_expr_cell(self, op, l, xs, prog, begin, end, out=None):
        if op not in (REDUCE_MAX, REDUCE_MIN):
            raise ValueError("unknown reduction %r" % (op,))
        _cell_layout(l, "field")
        if not 1 <= len(xs) <= FLUX_MAX_FIELDS:
            raise ValueError("%d fields" % len(xs))
        check_program(_prog_list(prog), len(xs))
        out = self.new_scalar() if out is None else out
        if _empty(begin, end):
            out[0] = -np.inf if op == REDUCE_MAX else np.inf
            return out
        if not _inside(l, begin, end, 0):
            raise ValueError("box leaves the allocation")
        vals = []
        for x in xs:
            a, ref = _view(l, x)
            vals.append(a[_sl(ref, begin, end)])
        with np.errstate(all="ignore"):
            v = eval_program(_prog_list(prog), vals)
        out[0] = float(np.max(v) if op == REDUCE_MAX else np.min(v))
        return out

    def apply_bc_cell(self, l, x, geom, kind, expr, face_mask):
        """EXAMG_BC_NEGATE: ghost = -interior on the faces of the mask, tangentially the inner cells only; the other kinds as before."""
        if kind != BC_NEGATE:
            return CellOracleOps.apply_bc_cell(self, l, x, geom, kind, expr, face_mask)
        a, ref = _view(l, x)
        for d in range(l.nd):
            for side in (0, 1):
                if not face_mask & (1 << (2 * d + side)):
                    continue
                if (l.ghost_r[d] if side else l.ghost_l[d]) < 1:
                    raise ValueError("face %d of dim %d has no ghost layer" % (side, d))
                b, e = [0, 0, 0], [1, 1, 1]
                for t in range(l.nd):
                    b[t], e[t] = 0, l.inner[t]
                if side == 0:
                    e[d] = 1
                else:
                    b[d] = l.inner[d] - 1
                off = [0, 0, 0]
                off[d] = 1 if side else -1
                gb, ge = _shift(b, e, off)
                a[_sl(ref, gb, ge)] = -a[_sl(ref, b, e)]
