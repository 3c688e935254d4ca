#!/usr/bin/env python
"""tests/golden/own/stokes{2,3}d.results from THIS repository's numpy restatement of the staggered-grid kernels (tests/mac_ops.py) -- "own
oracle", not reference data: the lines StokesSolver.Solve prints through reduced_prec (exastencils_amd/stokes.py) at the sizes the tests
run, 2-D levels 1 .. 5 (96^2 cells) and 3-D levels 1 .. 3 (24^3).  The reference's Stokes programs differ in the colouring of the box
sweep and in the coarse solver; their results files are not comparable.

Usage: python tests/golden/make_stokes_goldens.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mac_ops import MacOracleOps  # noqa: E402

from exastencils_amd.stokes import ConfigStokes, StokesSolver  # noqa: E402

SIZES = {2: 5, 3: 3}      # nd -> finest level

if __name__ == "__main__":
    for nd, hi in SIZES.items():
        S = StokesSolver(MacOracleOps(), ConfigStokes(nd=nd, max_level=hi))
        S.Solve()
        path = os.path.join(ROOT, "tests", "golden", "own", "stokes%dd.results" % nd)
        with open(path, "w") as f:
            f.write("\n".join(S.log) + "\n")
        print(path, "%d cycles" % S.iterations)
