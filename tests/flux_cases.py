"""TEST-ONLY: the cases shared by the flux tests (tests/test_flux.py on the CPU, tests/test_gpu_flux.py on the MI355X) and by
tools/flux_bench.py: the shallow-water step as a FluxSpec, an asymmetric spec that exercises every limit of examg_flux_t, shapes,
boxes, layouts and data."""
import numpy as np

from exastencils_amd.flux import FluxComp, FluxSpec, FluxTerm
from exastencils_amd.layout import FieldLayout

G = 9.81
C, E, W, N, S = (0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)
SENTINEL = -7.25e77

# cells x, y: the smallest at which window edges (62 written columns per wave), short rows and the ring of two rows can go wrong
SHAPES = [(8, 8), (66, 5), (130, 9), (257, 3)]


def push(k):
    return ("f%d" % k, None)


def const(v):
    return ("const", float(v))


def op(name):
    return (name, None)


# fields: 0 h, 1 hu, 2 hv, 3 b.  Only + - * /: every instruction is one IEEE rounding, the device must give numpy's bits.
SWE_F0 = [push(1)]
SWE_F1 = [push(1), push(1), op("*"), push(0), op("/"), const(0.5), const(G), op("*"), push(0), op("*"), push(0), op("*"), op("+")]
SWE_F2 = [push(1), push(2), op("*"), push(0), op("/")]
SWE_G0 = [push(2)]
SWE_G2 = [push(2), push(2), op("*"), push(0), op("/"), const(0.5), const(G), op("*"), push(0), op("*"), push(0), op("*"), op("+")]
SWE_S = [const(-0.5), const(G), op("*"), push(0), op("*"), push(3), op("*")]
WAVE_SPEED = [push(1), push(0), op("/"), op("fabs"), push(2), push(0), op("/"), op("fabs"), op("max"), const(G), push(0), op("*"), op("sqrt"),
              op("+")]
SURFACE = [push(0), push(3), op("+")]
CENTERING = ((W, E, S, N), (0.25, 0.25, 0.25, 0.25))


def swe_spec(sx=0.0123 * 0.5, sy=0.0117 * 0.5):
    """One Lax-Friedrichs step of the shallow-water equations; sx = (dt / dx) * 0.5, sy = (dt / dy) * 0.5."""
    progs = [SWE_F0, SWE_F1, SWE_F2, SWE_G0, SWE_G2, SWE_S]
    f0, f1, f2, g0, g2, s = range(6)
    return FluxSpec(progs, [
        FluxComp(0, *CENTERING, (FluxTerm(f0, E, W, -sx), FluxTerm(g0, N, S, -sy))),
        FluxComp(1, *CENTERING, (FluxTerm(f1, E, W, -sx), FluxTerm(f2, N, S, -sy), FluxTerm(s, E, W, sx))),
        FluxComp(2, *CENTERING, (FluxTerm(f2, E, W, -sx), FluxTerm(g2, N, S, -sy), FluxTerm(s, N, S, sy))),
    ])


def swe_data(rng, lin):
    """h in [5, 15], hu, hv in [-3, 3], b in [-11, -9] over the whole allocation (ghosts included)."""
    n = int(lin.size)
    return [rng.uniform(5.0, 15.0, n), rng.uniform(-3.0, 3.0, n), rng.uniform(-3.0, 3.0, n), rng.uniform(-11.0, -9.0, n)]


# -- the asymmetric set: six fields, the limits of the programs, terms between any two cells ---------------------------------------------
P_PUSH = [push(5)]                                                       # a single field push
P_LONG = [push(0)] + [x for k in range(15) for x in (push((k + 1) % 6), op("+-*"[k % 3]))] + [op("neg")]       # 32 instructions: the limit
P_DEEP = [push(k % 6) for k in range(8)] + [op(o) for o in "+*-+*-+"]      # 8 values on the stack: the limit
P_MIX = [push(2), push(3), op("*"), push(4), op("-")]
P_AXPY = [push(1), const(0.37), op("*"), push(4), op("+")]
assert len(P_LONG) == 32 and len(P_DEEP) == 15

ASYM_PROGS = [P_PUSH, P_LONG, P_DEEP, P_MIX, P_AXPY]
ASYM_COMPS = [
    FluxComp(3, (C, E, S), (0.3, -0.7, 1.9),
             (FluxTerm(1, E, C, 0.61), FluxTerm(2, C, S, -1.3), FluxTerm(0, N, W, 0.77), FluxTerm(3, W, N, 2.5))),      # a program per term
    FluxComp(5, (N,), (1.1,), ()),                                                                                      # no terms
    FluxComp(0, (E, W, C, N, S), (0.11, -0.23, 0.37, 0.53, -0.71), (FluxTerm(4, E, C, 1.0),)),
    FluxComp(2, (W, C), (0.5, -2.0), (FluxTerm(1, S, N, 0.1), FluxTerm(1, C, E, -0.2))),
]


def asym_spec(ncomp):
    return FluxSpec(ASYM_PROGS, ASYM_COMPS[:ncomp])


def asym_data(rng, lin):
    return [rng.uniform(0.5, 1.5, int(lin.size)) for _ in range(6)]


def layouts(shape, align):
    """The inputs with one ghost layer, the outputs with two: every argument is indexed through its own layout."""
    return FieldLayout.cell(2, shape, 1, align=align), FieldLayout.cell(2, shape, 2, align=align)


def boxes(shape):
    nx, ny = shape
    full = ([0, 0, 0], [nx, ny, 1])
    inner = ([1, 1, 0], [nx - 1, ny - 1, 1])
    one = ([nx // 2, ny // 2, 0], [nx // 2 + 1, ny // 2 + 1, 1])
    return [("full", full), ("interior", inner), ("cell", one)]


GOLDEN = "MatrixClassTests_2D_FV_SWE.results"       # tests/golden: the results file of the reference's shallow-water test, as data


def check_golden(lines):
    """The printed lines of swe2d.exa4 against the results file of Testing/MatrixClassTests/2D_FV_SWE: the same line sequence, the words
    and the iteration count (652) exactly, every number within 1e-5 relative -- one unit of the last of its six printed digits.  A
    number whose golden magnitude is below 1e-9 needs only be below 1e-9 itself: the two hMin values of rounding noise (3.0e-14,
    2.6e-12) on lines 21 and 22."""
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)) as f:
        gold = [l for l in f.read().split("\n") if l.strip()]
    assert len(gold) == 70 and len(lines) == len(gold), (len(lines), len(gold))
    assert "Total number of iterations: 652" in lines
    for i, (a, g) in enumerate(zip(lines, gold)):
        wa, wg = a.split(), g.split()
        assert len(wa) == len(wg), (i, a, g)
        for x, y in zip(wa, wg):
            try:
                v, w = float(x), float(y)
            except ValueError:
                assert x == y, (i, a, g)
                continue
            if g.startswith("Total"):
                assert x == y, (i, a, g)
            elif abs(w) < 1e-9:
                assert abs(v) < 1e-9, (i, a, g)
            else:
                assert abs(v - w) <= 1e-5 * abs(w), (i, a, g)


def box_mask(lay, b, e):
    """Boolean mask over the allocation of `lay`: the cells of [b, e)."""
    m = np.zeros((lay.tot(2), lay.tot(1), lay.tot(0)), dtype=bool)
    m[tuple(slice(b[d] + lay.ref(d), e[d] + lay.ref(d)) for d in (2, 1, 0))] = True
    return m.reshape(-1)
