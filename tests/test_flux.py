"""Explicit flux-form time steps in the ExaSlang-4 interpreter, on the CPU: `Expr` declarations and offset accesses in the parser, the
composition of offsets through nested Exprs, the flux loop as ONE flux_step with its programs, offsets and scales, every refusal by its
text, and examples/exa4/swe2d.exa4 on the numpy kernel layer (tests/flux_ops.py) against the results file of the reference's
shallow-water test (tests/golden, as data) -- interpreted, and with auto_graph on the recording stand-in of tests/graph_ops.py."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import flux_cases as K  # noqa: E402
from flux_ops import FluxOracleOps  # noqa: E402
from graph_ops import DeferringOps  # noqa: E402

from exastencils_amd import exa4  # noqa: E402
from exastencils_amd.exa4_conservation import expand  # noqa: E402
from exastencils_amd.exa4_parser import Exa4SyntaxError, Exa4Unsupported, Parser  # noqa: E402

EX = os.path.join(ROOT, "examples", "exa4")
E, W, N, S, C = (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 0)


def _swe(ops, **kw):
    return exa4.load(os.path.join(EX, "swe2d.exa4"), os.path.join(EX, "swe2d.knowledge"), ops=ops, **kw)


# -- parser ------------------------------------------------------------------------------------------------------------------------
SCOPES = """
Field q< global, L, None >[2]@all
Globals {
  Var dt : Real = 0.5
  Expr G = q * q
  Expr two@all = 2.0
}
Function F@all {
  Expr inFunction = G@east + two
  loop over q {
    Expr inLoop = inFunction@[0, 1]
    q<next> = inLoop@west - G@center
  }
}
"""


def test_expr_in_all_three_scopes_and_the_offset_aliases():
    ast = Parser(SCOPES).parse()
    assert [(n, lv) for n, lv, _ in ast.exprs] == [("G", None), ("two", ("all",))]
    assert ast.globals == [("dt", ("num", 0.5))]
    body = ast.functions[0].body
    assert body[0][:2] == ("exprdecl", "inFunction") and body[0][3][2] == ("off", ("id", "G", None), E)
    loop = body[1][5]
    assert loop[0] == ("exprdecl", "inLoop", None, ("off", ("id", "inFunction", None), N))
    assert loop[1][3] == ("bin", "-", ("off", ("id", "inLoop", None), W), ("off", ("id", "G", None), C))
    for alias, off in (("east", E), ("west", W), ("north", N), ("south", S), ("center", C)):
        e = Parser("Field q< global, L, None >@all\nFunction F@all {\n  Expr X = q\n  loop over q { q = X@%s }\n}\n" % alias).parse().functions[0].body[1][5][0][3]
        assert e == ("off", ("id", "X", None), off)
    # a field access takes an alias too; `@[..]` on a field stays what it was outside the ghost loops of boundary functions
    assert Parser("Field q< global, L, None >@all\nFunction F@all {\n  loop over q { q = q@east }\n}\n").parse().functions[0].body[0][5][0][3][0] == "off"
    with pytest.raises(Exa4Unsupported, match=r"line 3: offset access q@\[\.\.\.\]"):
        Parser("Field q< global, L, None >@all\nFunction F@all {\n  loop over q { q = q@[1, 0] }\n}\n").parse()
    ghost = Parser("Field q< global, L, None >@all\nFunction F@all {\n  loop over q only ghost [-1, 0] on boundary { q = -q@[1, 0] }\n}\n").parse()
    assert ghost.functions[0].body[0][5][0][3] == ("neg", ("off", ("fld", "q", None, None), E))
    with pytest.raises(Exa4Unsupported, match="offset access dt@east"):
        Parser("Globals {\n  Var dt : Real = 1\n}\nFunction F@all {\n  Var x : Real = dt@east\n}\n").parse()
    with pytest.raises(Exa4SyntaxError):      # an Expr has no type
        Parser("Globals {\n  Expr G : Real = 1\n}\n").parse()


def test_offsets_compose_by_addition_through_nested_exprs():
    q = ("fld", "q", None, None)
    defs = {"A": ("bin", "*", q, ("id", "s", None)), "B": ("bin", "+", ("off", ("id", "A", None), E), ("id", "A", None)),
            "V": ("bin", "*", ("id", "vf_cellWidth_x", None), q)}
    got = expand(("off", ("id", "B", None), N), defs)
    s = ("id", "s", None)      # scalars are untouched
    assert got == ("bin", "+", ("bin", "*", ("off", q, (1, 1, 0)), s), ("bin", "*", ("off", q, N), s))
    assert expand(("off", ("off", ("id", "A", None), E), W), defs) == ("bin", "*", q, s)      # east then west: the cell itself
    assert expand(("id", "V", None), defs) == defs["V"]
    with pytest.raises(Exa4Unsupported, match="virtual field vf_cellWidth_x read under the offset"):
        expand(("off", ("id", "V", None), E), defs)
    with pytest.raises(Exa4Unsupported, match="cycle"):
        expand(("id", "X", None), {"X": ("neg", ("id", "X", None))})


# -- the recogniser ------------------------------------------------------------------------------------------------------------------
class Recording(FluxOracleOps):
    def __init__(self):
        super().__init__()
        self.calls = []

    def flux_step(self, lin, ins, lout, outs, spec, begin, end):
        self.calls.append((ins, outs, spec, list(begin), list(end)))
        return super().flux_step(lin, ins, lout, outs, spec, begin, end)


def test_the_update_of_the_example_is_exactly_one_flux_step():
    ops = Recording()
    P = _swe(ops)
    P.call("Init", 8)
    before = P.launches
    P.call("Update", 8)
    assert P.launches == before + 1 and len(ops.calls) == 1
    ins, outs, spec, b, e = ops.calls[0]
    assert (b, e) == ([0, 0, 0], [256, 256, 1])
    h, hu, hv, bb = [P.fields[(n, 8)] for n in ("h", "hu", "hv", "b")]
    assert [t.data_ptr() for t in ins] == [x.data(x.active).data_ptr() for x in (h, hu, hv, bb)]
    assert [t.data_ptr() for t in outs] == [x.data(x.next).data_ptr() for x in (h, hu, hv)]
    # six programs: F2 and G1 are one expression, every other flux and the source are their own
    g5 = 0.5 * 9.81
    hu2, hv2 = [("f1", None), ("f1", None), ("*", None)], [("f2", None), ("f2", None), ("*", None)]
    ghh = [("const", g5), ("f0", None), ("f0", None), ("*", None), ("*", None), ("+", None)]
    F0, G0 = [("f1", None)], [("f2", None)]
    F1, G2 = hu2 + [("f0", None), ("/", None)] + ghh, hv2 + [("f0", None), ("/", None)] + ghh
    F2 = [("f1", None), ("f2", None), ("*", None), ("f0", None), ("/", None)]
    Sp = [("const", -0.5 * 9.81), ("f0", None), ("*", None), ("f3", None), ("*", None)]
    assert spec.programs == [F0, G0, F1, F2, Sp, G2]
    dx = 1000.0 / 256
    sx = (1.0e-5 / dx) * 0.5      # the scalar in the program's own association
    want = [(0, [(0, E, W, -sx), (1, N, S, -sx)]),
            (1, [(2, E, W, -sx), (3, N, S, -sx), (4, E, W, sx)]),
            (2, [(3, E, W, -sx), (5, N, S, -sx), (4, N, S, sx)])]
    assert len(spec.comps) == 3
    for comp, (field, terms) in zip(spec.comps, want):
        assert comp.field == field and comp.offsets == (E, W, N, S) and comp.coefs == (0.25,) * 4
        assert [(t.prog, t.plus, t.minus, t.scale) for t in comp.terms] == terms


MINI = """
Domain global< [0.0, 0.0] to [1.0, 1.0] >
Layout Halo< Real, Cell >@all {
  ghostLayers = [1, 1] with communication
  duplicateLayers = [0, 0] with communication
}
Field q< global, Halo, Neumann ( 1 ) >[2]@all
Field r< global, Halo, Neumann ( 1 ) >[2]@all
Field c< global, Halo, wall@finest ( ) >@all
Stencil Mean@all {
  [1, 0] => 0.5
  [-1, 0] => 0.5
}
Globals {
  Var dt : Real = 0.25
  Expr X = q * r
  Expr Y = q + r
}
Function wall@finest ( ) : Unit {
  loop over c only ghost [-1, 0] on boundary {
    c = -c@[1, 0]
  }
}
Function Step@finest {
  loop over q {
    q<next> = Mean * q - dt * ( X@east - X@west )
    r<next> = Mean * r + dt * ( Y@north - Y@south )
  }
}
Function Separate@finest {
  loop over q {
    q<next> = Mean * q - dt * ( X@east - X@west )
  }
  loop over r {
    r<next> = Mean * r + ( -dt ) * ( Y@south - Y@north ) - ( r@east - r )
  }
}
Function Application {
  apply bc to c@finest
  Step@finest ( )
}
"""


def _mini(text=MINI, nd=2, ops=None):
    return exa4.Exa4Program(text, dict(dimensionality=nd, minLevel=3, maxLevel=3), ops=ops or Recording())


def test_one_call_per_loop_and_the_sign_folded_into_the_scale():
    P = _mini()
    P.run()
    assert len(P.ops.calls) == 1 and len(P.ops.calls[0][2].comps) == 2
    P.call("Separate", 3)
    assert len(P.ops.calls) == 3
    one, two = P.ops.calls[1][2], P.ops.calls[2][2]
    assert [(t.plus, t.minus, t.scale) for t in one.comps[0].terms] == [(E, W, -0.25)]
    # a + (-k) * d and a - k * d are one call; a bare difference has the scale of its sign; a field access is its own program
    assert [(t.plus, t.minus, t.scale) for t in two.comps[0].terms] == [(S, N, -0.25), (E, C, -1.0)]
    assert two.programs == [[("f1", None), ("f0", None), ("+", None)], [("f0", None)]]      # the inputs in order of appearance: r, then q


REFUSALS = [
    ("3-D", 3, lambda t: t, "3-D flux loops"),
    ("node fields", 2, lambda t: t.replace("Real, Cell", "Real, Node").replace("duplicateLayers = [0, 0]", "duplicateLayers = [1, 1]")
     .replace("Neumann ( 1 )", "None").replace("wall@finest ( )", "None"), "flux loops over node fields"),
    ("not <next>", 2, lambda t: t.replace("q<next> = Mean * q - dt * ( X@east", "q = Mean * q - dt * ( X@east", 1), "is not the <next> slot"),
    ("one slot", 2, lambda t: t.replace("Field r< global, Halo, Neumann ( 1 ) >[2]", "Field r< global, Halo, Neumann ( 1 ) >"), "is not the <next> slot"),
    ("twice", 2, lambda t: t.replace("    r<next> = Mean * r + dt * ( Y@north - Y@south )", "    q<next> = Mean * q + dt * ( Y@north - Y@south )", 1), "appears twice"),
    ("reads <next>", 2, lambda t: t.replace("Expr Y = q + r", "Expr Y = q<next> + r"), "reads q<next>"),
    ("two expressions", 2, lambda t: t.replace("( X@east - X@west )", "( X@east - Y@west )", 1), "a difference of one expression at two axis cells"),
    ("no difference", 2, lambda t: t.replace("dt * ( X@east - X@west )", "dt * ( X@east + X@west )", 1), "a difference of one expression at two axis cells"),
    ("diagonal", 2, lambda t: t.replace("( X@east - X@west )", "( X@[1, 1] - X@west )", 1), "a difference of one expression at two axis cells"),
    ("reach 2", 2, lambda t: t.replace("Expr Y = q + r", "Expr Y = q@east + r"), "a difference of one expression at two axis cells"),
    ("first term", 2, lambda t: t.replace("q<next> = Mean * q - dt", "q<next> = q - dt", 1), "is not `S \\* Q`"),
    ("terms", 2, lambda t: t.replace("r<next> = Mean * r + dt * ( Y@north - Y@south )",
                                     "r<next> = Mean * r" + " + dt * ( Y@north - Y@south )" * 5, 1), "more than 4 difference terms"),
    ("programs", 2, lambda t: t.replace("  Expr Y = q + r\n", "  Expr Y = q + r\n" + "".join("  Expr Z%d = q * %d.0 + r\n" % (k, k) for k in range(9)))
     .replace("q<next> = Mean * q - dt * ( X@east - X@west )", "q<next> = Mean * q" + "".join(" + dt * ( Z%d@north - Z%d@south )" % (k, k) for k in range(4)), 1)
     .replace("r<next> = Mean * r + dt * ( Y@north - Y@south )", "r<next> = Mean * r" + "".join(" + dt * ( Z%d@north - Z%d@south )" % (k, k) for k in range(4, 8))
              + "\n    c<next> = Mean * c - ( Z8@east - Z8@west )", 1)
     .replace("Field c< global, Halo, wall@finest ( ) >@all", "Field c< global, Halo, wall@finest ( ) >[2]@all"),
     "more than 8 distinct point expressions"),
    ("fields", 2, lambda t: t.replace("Field c<", "".join("Field x%d< global, Halo, Neumann ( 1 ) >@all\n" % k for k in range(5)) + "Field c<")
     .replace("Expr Y = q + r", "Expr Y = q + r + x0 + x1 + x2 + x3 + x4"), "reads more than 6 fields"),
    ("ghost body", 2, lambda t: t.replace("c = -c@[1, 0]", "c = 2.0 * c@[1, 0]"), "the body of a ghost loop must be"),
    ("ghost cell", 2, lambda t: t.replace("c = -c@[1, 0]", "c = -c@[0, 1]"), "the body of a ghost loop must be"),
    ("solve locally", 2, lambda t: t.replace("    q<next> = Mean * q - dt * ( X@east - X@west )\n    r<next> = Mean * r + dt * ( Y@north - Y@south )",
                                             "    solve locally {\n      q<next> => q<next> + dt * ( X@east - X@west ) == Mean * q\n    }", 1),
     "solve locally as an explicit time step"),
    ("virtual field", 2, lambda t: t.replace("Expr X = q * r", "Expr X = vf_cellWidth_x * r"), "virtual field vf_cellWidth_x read under the offset"),
]


@pytest.mark.parametrize("name,nd,edit,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_by_name(name, nd, edit, text):
    src = edit(MINI)
    assert src != MINI or nd == 3
    if nd == 3:
        src = src.replace("[0.0, 0.0] to [1.0, 1.0]", "[0.0, 0.0, 0.0] to [1.0, 1.0, 1.0]").replace("[1, 1] with", "[1, 1, 1] with").replace(
            "[0, 0] with", "[0, 0, 0] with").replace("[1, 0] =>", "[1, 0, 0] =>").replace("[-1, 0] =>", "[-1, 0, 0] =>")
    ops = Recording()
    with pytest.raises(Exa4Unsupported, match=text):
        _mini(src, nd, ops).run()
    assert not ops.calls      # refused before anything is launched


def test_vector_fields_stay_refused():
    src = MINI.replace("Layout Halo< Real, Cell >", "Layout Halo< ColumnVector<Real,3>, Cell >")
    with pytest.raises(Exa4Unsupported, match="vector-valued"):
        _mini(src)


# -- the example -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interpreted():
    P = _swe(FluxOracleOps())
    P.run()
    return P


def test_swe2d_prints_the_golden_lines(interpreted):
    K.check_golden(interpreted.out)
    assert interpreted.globals["curTime"] >= 100.0


def test_swe2d_with_auto_graph_prints_the_same_text(interpreted):
    """Update reads the global dt, which changes every step: the guard of its recording makes every later call interpreted, never a
    stale replay.  AdvanceTimestep and the wall functions read no global and are replayed."""
    ops = DeferringOps(FluxOracleOps())
    P = _swe(ops, auto_graph=True)
    assert P.auto_graph
    P.run()
    assert P.out == interpreted.out
    assert ops.recordings >= 1 and P.graph_replays >= 1
    rec = P._auto_graphs.get(("Update", 8))
    assert rec and rec["replays"] == 1      # the recording's own replay, at the second call; no call since met its guard


# -- the kernels' registers -------------------------------------------------------------------------------------------------------------
def test_the_flux_kernels_use_no_scratch(tmp_path):
    """The point programs are interpreted from named registers: no indexed array, nothing spilled to memory.  The code-object metadata of
    kernels_flux.hip, compiled for the device with the flags of the build, says private segment 0 and no VGPR spill for every kernel."""
    import re
    import subprocess

    import __graft_entry__ as ge

    out = str(tmp_path / "flux.s")
    flags = [f for f in ge.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([os.environ.get("HIPCC", "hipcc")] + flags + ["--cuda-device-only", "-S", os.path.join(ge.CSRC, "kernels_flux.hip"), "-o", out],
                   check=True, capture_output=True)
    with open(out) as f:
        meta = f.read().split("amdhsa.kernels:")[1]
    kernels = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", meta)
    names = " ".join(k[0] for k in kernels)
    assert "k_flux_march" in names and "k_flux_gather" in names and "k_reduce_expr_partial" in names
    assert all(int(seg) == 0 and int(spill) == 0 for _, seg, spill in kernels), kernels
