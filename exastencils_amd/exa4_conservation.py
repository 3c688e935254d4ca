"""Explicit flux-form time steps on cell fields in the ExaSlang-4 interpreter (mixin of Exa4Program): `Expr` macros and their offset
accesses, the flux loop (`Q<next> = S * Q - s * ( F@east - F@west ) ..`: ONE examg_flux_step for the whole body), reductions over
point expressions of cell fields (examg_reduce_expr_cell) and the ghost loops of boundary functions (`hu = -hu@[1, 0]`: one face of
examg_apply_bc_cell).  Reference: Examples/SWE/2D_FV_SWE.exa4; baseExt/l4/L4_ExpressionDeclaration.scala, util/l4/L4_OffsetAlias.scala.
Everything here RECOGNISES: it hands back a LoopStmt record (exa4_statements.py) and launches nothing; the launcher issues the call."""
from __future__ import annotations

from .exa4_parser import Exa4Unsupported, _COORD, _GRIDW, _contains, _walk
from .exa4_statements import LoopStmt
from .flux import ZERO, FluxComp, FluxSpec, FluxTerm, field_program
from .lib import (BC_NEGATE, BC_NEUMANN, BC_VALUE_MINUS, FLUX_MAX_COMP, FLUX_MAX_ENTRIES, FLUX_MAX_FIELDS, FLUX_MAX_PROGS, FLUX_MAX_TERMS, MAX_NL_EXPR, NL_STACK,
                  REDUCE_MAX, REDUCE_MIN)

_EXPR = "__expr__"          # prefix of an `Expr` in the variables of a frame
_UNARY = {"sin": "sin", "cos": "cos", "exp": "exp", "sinh": "sinh", "cosh": "cosh", "sqrt": "sqrt", "tan": "tan", "log": "log", "fabs": "fabs",
          "abs": "fabs", "tanh": "tanh"}


def _add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def expand(node, defs, off=ZERO, depth=0):
    """The AST `node` with every name of `defs` (Expr macros) replaced by its definition, and the offsets of ("off", e, o) nodes added
    to every field access below them, through nested macros; a field access under a non-zero offset becomes ("off", fld, offset).
    Scalars are untouched; a virtual field of the grid under a non-zero offset is refused by name."""
    if depth > 32:
        raise Exa4Unsupported("Expr declarations that name each other in a cycle")
    if isinstance(node, list):
        return [expand(x, defs, off, depth) for x in node]
    if not isinstance(node, tuple) or not node or not isinstance(node[0], str):
        return node
    k = node[0]
    if k == "off":
        return expand(node[1], defs, _add(off, node[2]), depth)
    if k == "id" and len(node) == 3 and isinstance(node[1], str):
        if node[1] in defs:
            return expand(defs[node[1]], defs, off, depth + 1)
        if off != ZERO and (_COORD.match(node[1]) or _GRIDW.match(node[1]) or node[1].startswith("vf_")):
            raise Exa4Unsupported("virtual field %s read under the offset %s of an Expr" % (node[1], list(off)))
        return node
    if k == "vfo" and off != ZERO:
        raise Exa4Unsupported("virtual field %s read under the offset %s of an Expr" % (node[1], list(off)))
    if k == "fld":
        return node if off == ZERO else ("off", node, off)
    if k == "exprdecl":      # a definition is expanded where it is used
        return node
    return (k,) + tuple(expand(c, defs, off, depth) if isinstance(c, (tuple, list)) else c for c in node[1:])


def _strip(e):
    """(the expression with its offset accesses replaced by the plain field accesses, the set of offsets its field accesses stand under)."""
    offs = set()

    def rec(n):
        if isinstance(n, list):
            return [rec(x) for x in n]
        if not isinstance(n, tuple) or not n or not isinstance(n[0], str):
            return n
        if n[0] == "off":
            offs.add(tuple(n[2]))
            return n[1]
        if n[0] == "fld":
            offs.add(ZERO)
            return n
        return (n[0],) + tuple(rec(c) if isinstance(c, (tuple, list)) else c for c in n[1:])

    return rec(e), offs


def _signed_terms(e, sign=1.0):
    """The terms of a chain of + and -, left to right, each with its sign.  The chain is the left spine of the tree (the operators
    associate to the left): a right operand that is itself a sum or a difference stood in parentheses and is one term."""
    if e[0] == "bin" and e[1] in ("+", "-"):
        return _signed_terms(e[2], sign) + [(sign if e[1] == "+" else -sign, e[3])]
    if e[0] == "neg":
        return _signed_terms(e[1], -sign)
    return [(sign, e)]


def _axis(o) -> bool:
    return o[2:] in ((), (0,)) and (abs(o[0]) + abs(o[1])) <= 1


class Conservation:
    # -- Expr macros ----------------------------------------------------------------------------------------------------------
    def _global_exprs(self):
        return {name: e for name, _lv, e in self.ast.exprs}

    def _inline_global_exprs(self):
        """The global `Expr`s are macros: substituted into every function body once, at declaration -- from then on a function's text
        names the globals its macros read (what a recording of it depends on, exa4.py: _graph_deps).  A function that declares an
        Expr of the same name keeps its own."""
        defs = self._global_exprs()
        if not defs:
            return
        for fns in self.functions.values():
            for fn in fns:
                local = {n[1] for n in _walk(("block", list(fn.body))) if n and n[0] == "exprdecl"}
                fn.body = expand(fn.body, {k: v for k, v in defs.items() if k not in local})

    def _expr_defs(self, fr, body=()):
        """The Exprs in scope: those of the enclosing function and loop bodies (frame) and of this loop body."""
        defs = {k[len(_EXPR):]: v for k, v in fr.vars.items() if isinstance(k, str) and k.startswith(_EXPR)}
        for st in body:
            if st[0] == "exprdecl":
                defs[st[1]] = st[3]
        return defs

    def _expanded_body(self, body, fr):
        """The assignments of a loop body with Exprs substituted and `Val`s inlined (a Val of a loop body is a point expression)."""
        defs = self._expr_defs(fr, body)
        out = []
        for st in body:
            if st[0] == "exprdecl":
                continue
            if st[0] == "decl" and st[2] is not None:
                defs[st[1]] = expand(st[2], defs)
                continue
            out.append(expand(st, defs) if defs or _has_off(st) else st)
        return out

    # -- programs over cell fields ----------------------------------------------------------------------------------------------
    def _field_slot(self, e, fr, fields, what):
        """Index of the field access e among the inputs of the call (appended when new)."""
        F, s = self._field(e, fr)
        if not F.layout.is_cell:
            raise Exa4Unsupported("%s reads the node field %s (cell fields only)" % (what, F.name))
        if e[2] in ("next", "nextSlot") and F.num_slots > 1:
            raise Exa4Unsupported("%s reads %s<next>, a slot the loop writes" % (what, F.name))
        for k, (G, gs) in enumerate(fields):
            if G is F and gs == s:
                return k
        if len(fields) >= FLUX_MAX_FIELDS:
            raise Exa4Unsupported("%s reads more than %d fields" % (what, FLUX_MAX_FIELDS))
        fields.append((F, s))
        return len(fields) - 1

    def _compile_field_expr(self, e, fr, fields, what):
        """Postfix program over lib.FLUX_OPS of a point expression over cell fields at the cell: operands in the order of the tree,
        scalars evaluated on the host exactly where the tree has them."""
        k = e[0]
        if k == "num":
            return [("const", float(e[1]))]
        if k == "fld":
            return [("f%d" % self._field_slot(e, fr, fields, what), None)]
        if k == "off":
            raise Exa4Unsupported("%s: an offset access inside a point expression" % what)
        if self._is_scalar(e):
            return [("const", float(self._eval(e, fr)))]
        if k == "neg":
            return self._compile_field_expr(e[1], fr, fields, what) + [("neg", None)]
        if k == "bin" and e[1] in ("+", "-", "*", "/"):
            return self._compile_field_expr(e[2], fr, fields, what) + self._compile_field_expr(e[3], fr, fields, what) + [(e[1], None)]
        if k == "bin" and e[1] == "**":
            base = self._compile_field_expr(e[2], fr, fields, what)
            n = e[3][1] if e[3][0] == "num" else None
            if len(base) == 1 and n is not None and float(n) in (2.0, 3.0, 4.0):      # the generator expands small integer powers into products
                return base + (base + [("*", None)]) * (int(n) - 1)
            return base + self._compile_field_expr(e[3], fr, fields, what) + [("pow", None)]
        if k == "call" and e[1] not in self.functions:
            if e[1] in _UNARY and len(e[3]) == 1:
                return self._compile_field_expr(e[3][0], fr, fields, what) + [(_UNARY[e[1]], None)]
            if e[1] in ("pow", "max", "min") and len(e[3]) == 2:
                return self._compile_field_expr(e[3][0], fr, fields, what) + self._compile_field_expr(e[3][1], fr, fields, what) + [(e[1], None)]
        raise Exa4Unsupported("%s: point expression with %s %r" % (what, k, e[1] if len(e) > 1 else ""))

    @staticmethod
    def _check_program(prog, what):
        if len(prog) > MAX_NL_EXPR:
            raise Exa4Unsupported("%s: a point expression of %d instructions (limit %d)" % (what, len(prog), MAX_NL_EXPR))
        sp = deep = 0
        for name, _ in prog:
            sp += 1 if name == "const" or (name[0] == "f" and name[1:].isdigit()) else (-1 if name in ("+", "-", "*", "/", "pow", "max", "min") else 0)
            deep = max(deep, sp)
        if deep > NL_STACK:
            raise Exa4Unsupported("%s: a point expression that needs a stack of %d (limit %d)" % (what, deep, NL_STACK))

    # -- the flux loop ----------------------------------------------------------------------------------------------------------
    def _recognise_flux_loop(self, body, f, only, where, reduction, colour, fr):
        """LoopStmt('flux_step') for a loop body of assignments `Q<next> = S * Q +- s * ( X@a - X@b ) ..`, None when no assignment of
        the body reads anything at a neighbouring cell (the loop is none of this kind).  Refusals by name."""
        defs = self._expr_defs(fr, body)
        if not any(st[0] == "exprdecl" or _has_off(st) or _names(st, defs) for st in body):
            return None
        what = "flux loop over %s" % f.name
        if any(st[0] == "solve" for st in body):
            raise Exa4Unsupported("%s: solve locally as an explicit time step (write the update as assignments to the <next> slots)" % what)
        stmts = self._expanded_body(body, fr)
        if not any(_has_off(st) for st in stmts):
            return None
        if self.nd != 2:
            raise Exa4Unsupported("%s: %d-D flux loops (the 2-D kernels only are built)" % (what, self.nd))
        if not f.layout.is_cell:
            raise Exa4Unsupported("%s: flux loops over node fields" % what)
        if only is not None or where is not None or reduction is not None or colour is not None or fr.contract is not None:
            raise Exa4Unsupported("%s with an `only` region, a condition, a reduction, a colouring or under contraction" % what)
        fields, progs, comps, outs = [], [], [], []
        for st in stmts:
            if st[0] != "assign" or st[1] != "=" or st[2][0] != "fld":
                raise Exa4Unsupported("%s: a statement that is not an assignment `Q<next> = ..`" % what)
            D, ds = self._field(st[2], fr)
            if not D.layout.is_cell:
                raise Exa4Unsupported("%s: flux loops over node fields (%s)" % (what, D.name))
            if D.num_slots != 2 or st[2][2] not in ("next", "nextSlot"):
                raise Exa4Unsupported("%s: the destination %s is not the <next> slot of a field with two slots" % (what, D.name))
            if any(G is D for G, _ in outs):
                raise Exa4Unsupported("%s: the destination %s appears twice" % (what, D.name))
            if len(outs) >= FLUX_MAX_COMP:
                raise Exa4Unsupported("%s: more than %d assignments in one loop" % (what, FLUX_MAX_COMP))
            terms = _signed_terms(st[3])
            sign0, t0 = terms[0]
            m = self._sten_times_field(t0, fr) if sign0 > 0 else None
            if m is None or m[1] != "stencil" or m[0] != 1.0 or m[2].cfield is not None or getattr(m[2], "is_axis", False):
                raise Exa4Unsupported("%s: the first term of %s<next> is not `S * Q` with S a constant stencil" % (what, D.name))
            A = m[2]
            if len(A.offsets) < 1 or len(A.offsets) > FLUX_MAX_ENTRIES or not all(_axis(tuple(o)) for o in A.offsets):
                raise Exa4Unsupported("%s: the stencil of %s<next> has entries off the axes, of reach 2 or more than %d" % (what, D.name, FLUX_MAX_ENTRIES))
            q = self._field_slot(m[4], fr, fields, what)
            fterms = []
            for sign, t in terms[1:]:
                scale, diff = sign, t
                if t[0] == "bin" and t[1] == "*":
                    if self._is_scalar(t[2]) and not _has_off(t[2]):
                        scale, diff = sign * float(self._eval(t[2], fr)), t[3]
                    elif self._is_scalar(t[3]) and not _has_off(t[3]):
                        scale, diff = sign * float(self._eval(t[3], fr)), t[2]
                bad = Exa4Unsupported("%s: a term of %s<next> is not scalar * ( X@a - X@b ), a difference of one expression at two axis cells" % (what, D.name))
                if diff[0] != "bin" or diff[1] != "-":
                    raise bad
                (xa, oa), (xb, ob) = _strip(diff[2]), _strip(diff[3])
                if xa != xb or len(oa) != 1 or len(ob) != 1:
                    raise bad
                a, b = next(iter(oa)), next(iter(ob))
                if not _axis(a) or not _axis(b):
                    raise bad
                if len(fterms) >= FLUX_MAX_TERMS:
                    raise Exa4Unsupported("%s: more than %d difference terms in %s<next>" % (what, FLUX_MAX_TERMS, D.name))
                prog = self._compile_field_expr(xa, fr, fields, what)
                self._check_program(prog, what)
                if prog not in progs:
                    if len(progs) >= FLUX_MAX_PROGS:
                        raise Exa4Unsupported("%s: more than %d distinct point expressions" % (what, FLUX_MAX_PROGS))
                    progs.append(prog)
                fterms.append(FluxTerm(progs.index(prog), a, b, scale))
            comps.append(FluxComp(q, tuple(tuple(o) for o in A.offsets), tuple(float(c) for c in A.coefs), tuple(fterms)))
            outs.append((D, ds))
        for (G, gs) in fields:
            if any(G is D and gs == ds for D, ds in outs):
                raise Exa4Unsupported("%s reads %s<next>, a slot the loop writes" % (what, G.name))
            if G.layout != fields[0][0].layout:
                raise Exa4Unsupported("%s: the fields read have different layouts (%s, %s)" % (what, fields[0][0].name, G.name))
        for D, _ in outs:
            if D.layout != outs[0][0].layout:
                raise Exa4Unsupported("%s: the fields written have different layouts (%s, %s)" % (what, outs[0][0].name, D.name))
        return LoopStmt("flux_step", outs[0][0], outs[0][1], prog=(fields, outs, FluxSpec(progs, comps)))

    # -- reductions over point expressions ------------------------------------------------------------------------------------------
    def _recognise_reduce_expr(self, op, var, st, locals_, f, fr):
        """LoopStmt('reduce_expr') for `v = max | min ( v, E )`, E a point expression over cell fields at the cell (Vals inlined)."""
        rhs = st[3]
        if op not in ("max", "min") or st[1] != "=" or rhs[0] != "call" or rhs[1] != op or len(rhs[3]) != 2:
            return None
        other = [a for a in rhs[3] if a != ("id", var, None)]
        if len(other) != 1 or not f.layout.is_cell:
            return None
        defs = self._expr_defs(fr)
        for name, e in locals_.items():
            if e is not None:
                defs[name] = expand(e, defs)
        E = expand(other[0], defs)
        what = "reduction %s over %s" % (op, f.name)
        if _has_off(E):
            raise Exa4Unsupported("%s: a point expression read at a neighbouring cell" % what)
        fields = []
        prog = self._compile_field_expr(E, fr, fields, what)
        self._check_program(prog, what)
        if not fields:
            return None
        for G, _ in fields:
            if G.layout != fields[0][0].layout:
                raise Exa4Unsupported("%s: the fields read have different layouts (%s, %s)" % (what, fields[0][0].name, G.name))
        if self.domain.world_size != 1:
            raise Exa4Unsupported("%s on %d blocks (world_size must be 1)" % (what, self.domain.world_size))
        return LoopStmt("reduce_expr", fields[0][0], fields[0][1], s=float(REDUCE_MAX if op == "max" else REDUCE_MIN), prog=(fields, field_program(prog)))

    # -- boundary functions ---------------------------------------------------------------------------------------------------------
    def _recognise_ghost_loop(self, s, f, fr):
        """LoopStmt('bc_face') for `loop over F only ghost [d] on boundary { F = [-] F@[-d] }` or `{ F = E - F@[-d] }` on a cell field:
        the Neumann kind, the reflecting wall or the value-minus-interior kind of examg_apply_bc_cell on one face (prog: kind, face bit,
        program of E or None); None for every loop that is not a ghost loop of a cell field."""
        _, target, only, where, reduction, body = s
        if only is None or only[0] != "ghost" or not f.layout.is_cell:
            return None
        what = "loop over %s only ghost %s" % (f.name, list(only[1]))
        d = tuple(only[1]) + (0,) * (3 - len(only[1]))
        nz = [t for t in range(3) if d[t] != 0]
        if not only[2] or len(nz) != 1 or nz[0] >= self.nd or abs(d[nz[0]]) != 1 or where is not None or reduction is not None:
            raise Exa4Unsupported("%s: ghost loops of cell fields are boundary functions -- one axis direction, `on boundary`, no condition" % what)
        bad = Exa4Unsupported("%s: the body of a ghost loop must be `%s = %s@[..]`, `%s = -%s@[..]` or `%s = E - %s@[..]` (E a value or a point "
                              "expression) with the cell inside the face" % ((what,) + (f.name,) * 6))
        stmts = self._expanded_body(body, fr)
        if len(stmts) != 1 or stmts[0][0] != "assign" or stmts[0][1] != "=" or stmts[0][2][0] != "fld":
            raise bad
        D, ds = self._field(stmts[0][2], fr)
        rhs, kind, E = stmts[0][3], BC_NEUMANN, None
        if rhs[0] == "neg":
            rhs, kind = rhs[1], BC_NEGATE
        elif rhs[0] == "bin" and rhs[1] == "-" and rhs[3][0] == "off" and rhs[3][1][0] == "fld":
            rhs, kind, E = rhs[3], BC_VALUE_MINUS, rhs[2]
        if rhs[0] != "off" or rhs[1][0] != "fld" or D is not f or self._field(rhs[1], fr) != (D, ds):
            raise bad
        if tuple(rhs[2]) + (0,) * (3 - len(rhs[2])) != tuple(-x for x in d):
            if E is None:
                raise bad
            raise Exa4Unsupported("%s: `%s = E - %s@%s` reads a cell that is not the one inside the face (%s)"
                                  % (what, f.name, f.name, list(rhs[2]), [-x for x in d[:len(rhs[2])]]))
        prog = None
        if E is not None:
            if _contains(E, ("fld", "sten", "sentry")):
                raise Exa4Unsupported("%s: a field access inside the value E of `%s = E - %s@[..]`" % (what, f.name, f.name))
            if _has_off(E) or _contains(E, ("vfo",)):
                raise Exa4Unsupported("%s: the value E of `%s = E - %s@[..]` with an offset access" % (what, f.name, f.name))
            prog = self._ghost_value_program(E, D.level, fr)
        face = 1 << (2 * nz[0] + (1 if d[nz[0]] > 0 else 0))
        if self.domain.neighbor(nz[0], d[nz[0]]) is not None:
            face = 0      # an interior face: `on boundary` leaves nothing to do
        return LoopStmt("bc_face", D, ds, prog=(kind, face, prog))

    def _ghost_value_program(self, E, lvl, fr):
        """The program of the value of a ghost loop (EXAMG_BC_VALUE_MINUS): evaluated at the ghost cell itself -- vf_cellCenter_* its centre,
        vf_nodePosition_* the node of its own index (EXAMG_OP_NODE_*); a value without a position is a one-instruction program."""
        from .lib import ExprC

        if not self._over_position(E):
            return ExprC.from_program([("const", float(self._eval(E, fr)))])
        for n in _walk(E):
            if n and n[0] == "id" and isinstance(n[1], str) and n[1].startswith("vf_boundary"):
                raise Exa4Unsupported("%s in the value of a ghost loop (the value is taken at the ghost cell, not on the face)" % n[1])
        key = ("ghostexpr", repr(E), lvl)
        if key not in self._fn_cache:
            self._node_ops = True      # _compile_point_expr: vf_nodePosition_* as the node-position opcodes
            try:
                self._fn_cache[key] = ExprC.from_program(self._compile_point_expr(E, lvl))
            except ValueError as ex:
                raise Exa4Unsupported(str(ex))
            finally:
                self._node_ops = False
        return self._fn_cache[key]

    def _merge_bc_faces(self, first: LoopStmt, fr):
        """The ghost loops that follow `first` in the function body being executed and go into its launch: consecutive bc_face statements
        of one function body that write distinct faces of the same field and slot, with nothing but startTimer / stopTimer of one timer
        between them.  Returns the records (first included); the loops taken are skipped when the body reaches them."""
        group = [first]
        if not self.fuse or not self._cont or not self._cont[-1][4]:
            return group
        body, i = self._cont[-1][0], self._cont[-1][1]
        faces, timer, taken = first.prog[1], None, []
        j = i + 1
        while j < len(body):
            st = body[j]
            if st[0] == "callstmt" and st[1][0] == "call" and st[1][1] in ("startTimer", "stopTimer") and st[1][1] not in self.functions:
                name = repr(st[1][3])
                if timer is not None and name != timer:
                    break
                timer = name
                j += 1
                continue
            if st[0] != "loop":
                break
            try:
                g, _ = self._field(st[1], fr)
                k = self._recognise_ghost_loop(st, g, fr)
            except Exa4Unsupported:
                break      # the body meets the statement itself and names the refusal
            if k is None or k.D is not first.D or k.ds != first.ds or (k.prog[1] & faces):
                break
            faces |= k.prog[1]
            group.append(k)
            taken.append(id(st))
            timer = None
            j += 1
        self._bc_taken = set(taken)
        return group


def _has_off(node) -> bool:
    return any(n and n[0] == "off" for n in _walk(node))


def _names(node, defs) -> bool:
    return bool(defs) and any(n and n[0] == "id" and n[1] in defs for n in _walk(node))
