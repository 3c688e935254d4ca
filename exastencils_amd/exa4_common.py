"""Names shared by the modules of the ExaSlang-4 interpreter (exastencils_amd/exa4*.py): loop kinds, the python mirror of the
built-in point functions (recognition only), frames and the return signal."""
from __future__ import annotations

import math
import os
import random
import re
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

from . import knowledge as _knowledge
from .comm import Communicator
from .domain import RectDomain
from .field import Field, Stencil
from .layout import FieldLayout
from .exa4_parser import (Exa4SyntaxError, Exa4Unsupported, FunctionDecl, Parser, _COORD, _GRIDW, _MATH, _arith,  # noqa: F401
                          _colour_cond, _conjuncts, _const_value, _contains, _find_calls, _has_coord, _lower_cond, _parity_expr, _walk)

APPLY, RESIDUAL, SMOOTH = 0, 1, 2


# =====================================================================================================================
# analytic point functions: python mirror of eval_fn (exastencils_amd/csrc/examg_common.h), used for recognition only
# =====================================================================================================================
def fn_eval(fn: int, p: Sequence[float], x: float, y: float, z: float) -> float:
    PI = math.pi
    k = p[0] if p else 0.0
    if fn == 0:
        return 0.0
    if fn == 1:
        return ((x * x) - ((0.5 * y) * y)) - ((0.5 * z) * z)
    if fn == 2:
        return math.cos(PI * x) - math.sin((2.0 * PI) * y)
    if fn == 3:
        return (PI * PI) * math.cos(PI * x) - ((4.0 * (PI * PI)) * math.sin((2.0 * PI) * y))
    if fn == 4:
        return k * (((x - (x * x)) * (y - (y * y))) * (z - (z * z)))
    if fn == 5:
        return (2.0 * k) * ((((x - (x * x)) * (y - (y * y))) + ((x - (x * x)) * (z - (z * z)))) + ((y - (y * y)) * (z - (z * z))))
    if fn == 6:
        return 1.0 - math.exp((-1.0 * k) * (((x - (x * x)) * (y - (y * y))) * (z - (z * z))))
    if fn == 7:
        return math.exp(k * (((x - (x * x)) * (y - (y * y))) * (z - (z * z))))
    if fn == 8:
        return (math.sin(PI * x) * math.sin(PI * y)) * math.sinh((math.sqrt(2.0) * PI) * z)
    if fn == 9:
        return (math.sin(PI * x) * math.sin(PI * y)) * math.sin(PI * z)
    if fn == 10:
        return k * ((x - (x * x)) * (y - (y * y)))
    if fn == 11:
        return (2.0 * k) * ((x - (x * x)) + (y - (y * y)))
    if fn == 12:
        return 1.0 - math.exp((-1.0 * k) * ((x - (x * x)) * (y - (y * y))))
    if fn == 13:
        return math.exp(k * ((x - (x * x)) * (y - (y * y))))
    if fn == 14:
        return (x * x) - (y * y)
    if fn == 15:
        return math.sin(PI * x) * math.sinh(PI * y)
    if fn == 16:
        return x * x
    raise ValueError("function id %d" % fn)


_FN_WITH_PARAM = {4, 5, 6, 7, 10, 11, 12, 13}
_FN_2D_ONLY = {2, 3, 10, 11, 12, 13, 14, 15}     # ignore z
_FN_ANY_DIM = {0, 16}
_N_FN = 17


# =====================================================================================================================
# frames
# =====================================================================================================================
class _Return(Exception):
    def __init__(self, value):
        self.value = value


@dataclass
class _Frame:
    level: Optional[int]
    vars: Dict[str, object]
    colour: Optional[int] = None
    mcolour: Optional[object] = None     # inside `color with` of a multi-colouring: the Colouring with the remainders of the current colour
    contract: Optional[tuple] = None     # (extent, posExt, negExt) inside `repeat .. with contraction`: loops widen at interior faces
