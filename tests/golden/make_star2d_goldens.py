#!/usr/bin/env python
"""tests/golden/own/jacobi2d_cell.results: what examples/exa4/jacobi2d_cell.exa4 prints with its own knowledge file -- "own oracle", not
reference data.  The program runs in the interpreter on the numpy restatement of the kernel layer (tests/star2d_ops.py on top of
tests/cell_ops.py and the C oracle): the residual norm at the start and after every 10th Jacobi step, then the step count.

Usage: python tests/golden/make_star2d_goldens.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from star2d_ops import Star2dOracleOps  # noqa: E402

from exastencils_amd import exa4  # noqa: E402

EX = os.path.join(ROOT, "examples", "exa4")
OUT = os.path.join(ROOT, "tests", "golden", "own")


def main():
    P = exa4.load(os.path.join(EX, "jacobi2d_cell.exa4"), os.path.join(EX, "jacobi2d_cell.knowledge"), ops=Star2dOracleOps())
    out = P.run()
    with open(os.path.join(OUT, "jacobi2d_cell.results"), "w") as f:
        f.write("\n".join(out) + "\n")
    print("jacobi2d_cell:", " ".join(out))


if __name__ == "__main__":
    main()
