"""Cases shared by the CPU and GPU tests of axis-aligned non-uniform grids (include/examg.h: examg_axis_op and the _grid entry points):
random node tables that differ per axis, the finite-difference and finite-volume stencils written over the grid's virtual fields, a
full reach-1 stencil with random tables, layouts in which every argument has ghost and pad widths of its own, and the two example
programs with their knowledge files."""
import os

import numpy as np

import nonlinear_cases as N

from exastencils_amd import knowledge
from exastencils_amd.exa4_parser import Parser, _const_value
from exastencils_amd.grid import GHOST, AxisGrid, AxisStencil, separate

ROOT = N.ROOT
EX = N.EX
OWN = os.path.join(N.GOLDEN, "own")
LVL = 0       # the level the random grids live on


def random_grid(nd, cells, seed):
    """Node tables of cumulated random widths, another range per axis (mutually different, positive, not dyadic)."""
    rng = np.random.default_rng(seed)
    nodes = {}
    for d in range(nd):
        w = rng.uniform(0.4 + 0.3 * d, 1.7 + 0.5 * d, cells[d] + 2 * GHOST) / (3.0 + d)
        nodes[(LVL, d)] = np.concatenate(([0.0], np.cumsum(w))) - 0.37 * (d + 1)
    return AxisGrid.from_nodes(nd, nodes)


def _offset(nd, d, o):
    v = ["0"] * nd
    v[d] = str(o)
    return "[" + ", ".join(v) + "]"


def fd_text(nd):
    """The stencil of examples/exa4/poisson{2,3}d_nonuniform.exa4."""
    ax = "xyz"[:nd]
    hm = ["vf_cellWidth_%s@%s" % (ax[d], _offset(nd, d, -1)) for d in range(nd)]
    h0 = ["vf_cellWidth_%s@%s" % (ax[d], _offset(nd, d, 0)) for d in range(nd)]
    lo = ["2.0 / ( %s * ( %s + %s ) )" % (hm[d], h0[d], hm[d]) for d in range(nd)]
    up = ["2.0 / ( %s * ( %s + %s ) )" % (h0[d], h0[d], hm[d]) for d in range(nd)]
    centre = " + ".join(t for d in range(nd) for t in (lo[d], up[d]))
    rows = ["%s => ( %s )" % (_offset(nd, 0, 0), centre)]
    for d in range(nd):
        rows += ["%s => -%s" % (_offset(nd, d, -1), lo[d]), "%s => -%s" % (_offset(nd, d, 1), up[d])]
    return "Stencil S@all {\n" + "\n".join(rows) + "\n}\n"


def fv_text(nd):
    """The stencil of Examples/Poisson/{2,3}D_FV_Poisson_fromL4.exa4: face area over the distance of the cell centres."""
    ax = "xyz"[:nd]

    def area(d):
        o = ["vf_cellWidth_%s" % ax[t] for t in range(nd) if t != d]
        return o[0] if nd == 2 else "( %s * %s )" % (o[0], o[1])

    def dist(d, a, b):
        return "( 0.5 * ( vf_cellWidth_%s@%s + vf_cellWidth_%s@%s ) )" % (ax[d], _offset(nd, d, a), ax[d], _offset(nd, d, b))

    lo = ["%s / %s" % (area(d), dist(d, 0, -1)) for d in range(nd)]
    up = ["%s / %s" % (area(d), dist(d, 1, 0)) for d in range(nd)]
    centre = " + ".join(t for d in range(nd) for t in (lo[d], up[d]))
    rows = ["%s => ( %s )" % (_offset(nd, 0, 0), centre)]
    for d in range(nd):
        rows += ["%s => -%s" % (_offset(nd, d, -1), lo[d]), "%s => -%s" % (_offset(nd, d, 1), up[d])]
    return "Stencil S@all {\n" + "\n".join(rows) + "\n}\n"


def entries(text):
    return Parser(text).parse().stencils[0].entries


def separated(text, nd, grid, lvl=LVL):
    return separate("S", entries(text), nd, lvl, grid, _const_value)


def permuted(st, order):
    """The same stencil with its entries (and their terms) in another declared order."""
    terms = [(new, s, tab) for new, old in enumerate(order) for e, s, tab in st.terms if e == old]
    return AxisStencil([st.offsets[k] for k in order], terms, st.tables, st.tab_begin, st.wform)


def full_stencil(nd, cells, seed, two_term_entries):
    """All 3^nd entries of reach 1 in a shuffled order, the first `two_term_entries` of them with two terms, tables and scalars random: the
    centre dominant and positive (the smoother divides by it), every term with its own pick of tables, some without a table of an axis."""
    rng = np.random.default_rng(seed)
    offs = [(a, b, c) for c in ((-1, 0, 1) if nd == 3 else (0,)) for b in (-1, 0, 1) for a in (-1, 0, 1)]
    offs = [offs[i] for i in rng.permutation(len(offs))]
    ntab = 5
    tables = [[rng.uniform(0.6, 1.4, cells[d] + 1) for _ in range(ntab)] if d < nd else [] for d in range(3)]
    terms = []
    for k, o in enumerate(offs):
        for j in range(2 if k < two_term_entries else 1):
            tab = tuple(int(rng.integers(-1, ntab)) if d < nd else -1 for d in range(3))
            s = float(rng.uniform(0.2, 0.9)) * (40.0 if o == (0, 0, 0) else -1.0)
            terms.append((k, s, tab))
    return AxisStencil(offs, terms, tables)


def layouts(nd, shape):
    """(lu, lf, ld): u one ghost layer, rhs none and rows padded to 2, dst one and rows padded to 16."""
    lu, _, lf, ld = N.layouts(nd, shape)
    return lu, lf, ld


def own_knowledge(nd, **over):
    k = knowledge.parse_file(os.path.join(EX, "poisson%dd_nonuniform.knowledge" % nd))
    k.update(over)
    return k


def own_text(nd):
    return N.text("poisson%dd_nonuniform.exa4" % nd)


def own_results(nd):
    with open(os.path.join(OWN, "poisson%dd_nonuniform.results" % nd)) as f:
        return f.read().split()


def run_own(nd, ops, **over):
    from exastencils_amd import exa4

    kw = {k: over.pop(k) for k in list(over) if k in ("fuse", "auto_graph")}
    P = exa4.Exa4Program(own_text(nd), own_knowledge(nd, **over), ops=ops, **kw)
    return P, P.run()
