"""Field layouts: the reference's per-dimension regions, kept verbatim because they are the
drop-in contract (Compiler/src/exastencils/field/ir/IR_FieldLayout.scala:30-129):

    pad | ghost | dup | inner | dup | ghost | pad        x fastest, referenceOffset = pad_l + ghost_l

Iterator coordinates (what `loop over` bodies and the kernels' begin/end use) put 0 at the lower
duplicate node; array index = iterator + referenceOffset.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence, Tuple

from .lib import LayoutC


FACE_LOCALIZATIONS = ("face_x", "face_y", "face_z")


@dataclass(frozen=True)
class FieldLayout:
    nd: int
    inner: Tuple[int, int, int]
    ghost: Tuple[int, int, int]
    dup: Tuple[int, int, int]
    pad_l: Tuple[int, int, int] = (0, 0, 0)
    pad_r: Tuple[int, int, int] = (0, 0, 0)
    communicates_dup: bool = True      # `duplicateLayers = [...] with communication`
    communicates_ghost: bool = True    # `ghostLayers = [...] with communication`
    # layout transformation of the program's `LayoutTransformations` block (include/examg.h: EXAMG_LAYOUT_*): 1 = the colour split
    # `[x, y, z] => [x / 2, y, z, x % 2]` (Testing/LayoutTrafo/rbgs.exa4:2).  Regions, iterator coordinates and boxes stay those of the
    # untransformed layout; only where a value lives changes.
    transform: int = 0
    # "node" | "cell" | "face_x" | "face_y" | "face_z": Python-side only.  The C struct is the same for all (a cell layout is the one without
    # duplicate layers, a face layout has them on its own axis only); the localization travels as the choice of entry point (examg_*_cell,
    # examg_*_face with the axis).
    localization: str = "node"
    # "real" | "complex": Python-side only, like the localization.  A point of a complex field is two consecutive doubles (re, im); every
    # count of the layout stays in POINTS and the element kind travels as the choice of entry point (examg_c*: include/examg.h).
    element: str = "real"
    # components of a vector-valued field (`Layout X< Vec2, Cell >`): Python-side only.  The C struct is the scalar one; component c of a
    # field lives at c * size doubles (the component is the slowest array dimension, field/l4/L4_FieldLayout.scala:63-73) and the count
    # travels as the argument n of the examg_vec_* entry points.
    ncomp: int = 1

    @property
    def is_vector(self) -> bool:
        return self.ncomp > 1

    def as_vector(self, n: int) -> "FieldLayout":
        """This layout for a column vector of n components per cell."""
        from dataclasses import replace

        if n not in (2, 3):
            raise ValueError("vector-valued fields have 2 or 3 components, not %r" % (n,))
        if not self.is_cell or self.transform or self.is_complex:
            raise ValueError("vector-valued fields are real cell fields in the untransformed layout")
        return replace(self, ncomp=int(n))

    def scalar(self) -> "FieldLayout":
        """The layout of one component."""
        from dataclasses import replace

        return replace(self, ncomp=1) if self.ncomp > 1 else self

    @property
    def is_cell(self) -> bool:
        return self.localization == "cell"

    @property
    def is_face(self) -> bool:
        return self.localization in FACE_LOCALIZATIONS

    @property
    def face_axis(self):
        """The axis a face field's faces are normal to; None for node and cell layouts."""
        return FACE_LOCALIZATIONS.index(self.localization) if self.is_face else None

    @property
    def is_complex(self) -> bool:
        return self.element == "complex"

    @property
    def doubles(self) -> int:
        """Doubles of an array of this layout: size points, two doubles each for a complex field."""
        return (2 if self.is_complex else 1) * self.ncomp * self.size

    def as_complex(self) -> "FieldLayout":
        from dataclasses import replace

        if self.transform or self.is_cell:
            raise ValueError("complex fields are node fields in the untransformed layout")
        return replace(self, element="complex")

    def real_view(self) -> "FieldLayout":
        """A complex field seen as a real field: every x count doubled.  `set` to a real constant, copies and pack / unpack of a complex
        field are the real entry points on this view, with the x bounds of the box doubled (real_view_box)."""
        from dataclasses import replace

        if not self.is_complex:
            return self

        def dx(t):
            return (2 * t[0], t[1], t[2])

        return replace(self, inner=dx(self.inner), ghost=dx(self.ghost), dup=dx(self.dup), pad_l=dx(self.pad_l), pad_r=dx(self.pad_r), element="real")

    @staticmethod
    def real_view_box(begin, end):
        return [2 * begin[0], begin[1], begin[2]], [2 * end[0], end[1], end[2]]

    @staticmethod
    def cell(nd: int, ncells: Sequence[int], ghost: int, communicates_ghost: bool = True, align: int = 0) -> "FieldLayout":
        """`Layout X< Real, Cell >`: no duplicate layers, inner = the cells (fragLen * 2^level per dimension).  `align`: pads x
        (as FieldLayout.node does) so that the first inner cell and the row length are multiples of `align` doubles -- with
        align = 2 the fine pair (2I, 2I+1) of every row of a cell field starts 16-byte aligned (the 16-byte form of
        examg_restrict_cell / examg_prolong_add_cell)."""
        inner = tuple(int(ncells[d]) if d < nd else 1 for d in range(3))
        if any(i < 1 for i in inner):
            raise ValueError("a Cell field needs at least one cell per dimension")
        g = tuple(ghost if d < nd else 0 for d in range(3))
        pl, pr = [0, 0, 0], [0, 0, 0]
        if align:
            pl[0] = (align - g[0] % align) % align
            tot = pl[0] + g[0] + inner[0] + g[0]
            pr[0] = (align - tot % align) % align
        return FieldLayout(nd, inner, g, (0, 0, 0), tuple(pl), tuple(pr), True, communicates_ghost, localization="cell")

    @staticmethod
    def face(nd: int, ncells: Sequence[int], axis: int, ghost: int, communicates_dup: bool = True, communicates_ghost: bool = True,
             align: int = 0) -> "FieldLayout":
        """`Layout X< Real, Face_x >` (fieldlike/l4/L4_FieldLikeLayoutDecl.scala:53-57): on `axis` like a node field, one duplicate layer
        per side and inner = cells - 1; on the other axes like a cell field, no duplicate layer and inner = cells.  Iterator coordinate 0
        on the own axis is the lower boundary face; face i is the lower face of cell i; `loop over` covers [0, cells + 1) on the own
        axis and [0, cells) on the others.  `align` pads x as FieldLayout.node / FieldLayout.cell do."""
        if not 0 <= axis < nd:
            raise ValueError("a %d-D field has no faces of axis %r" % (nd, axis))
        if any(int(ncells[d]) < 1 for d in range(nd)):
            raise ValueError("a Face field needs at least one cell per dimension")
        du = tuple(1 if d == axis else 0 for d in range(3))
        inner = tuple((int(ncells[d]) - du[d]) if d < nd else 1 for d in range(3))
        g = tuple(ghost if d < nd else 0 for d in range(3))
        pl, pr = [0, 0, 0], [0, 0, 0]
        if align:
            pl[0] = (align - g[0] % align) % align
            tot = pl[0] + g[0] + du[0] + inner[0] + du[0] + g[0]
            pr[0] = (align - tot % align) % align
        return FieldLayout(nd, inner, g, du, tuple(pl), tuple(pr), communicates_dup, communicates_ghost, localization=FACE_LOCALIZATIONS[axis])

    @property
    def ncells(self) -> Tuple[int, ...]:
        """Cells per axis of the block the field lives on."""
        return tuple(self.inner[d] + self.dup[d] for d in range(self.nd))

    def loop_box(self):
        """The box of `loop over` the field: the duplicate and inner points, no ghost."""
        return [0, 0, 0], [self.idx("DRE", d) if d < self.nd else 1 for d in range(3)]

    @staticmethod
    def node(nd: int, ncells: Sequence[int], ghost: int, communicates_dup: bool = True,
             communicates_ghost: bool = True, align: int = 0) -> "FieldLayout":
        """`Layout X< Real, Node >`: one duplicate layer per side, inner = cells + 1 - 2*dup
        (fieldlike/l4/L4_FieldLikeLayoutDecl.scala:49-51).  `align` = simd_vectorSize of
        IR_AddPaddingToFieldLayouts (field/ir/IR_AddPaddingToFieldLayouts.scala:36-41): pads x so
        that the first duplicate point and the row length are multiples of `align` doubles."""
        inner = tuple((int(ncells[d]) - 1) if d < nd else 1 for d in range(3))
        if any(i < 0 for i in inner):
            raise ValueError("a Node field needs at least one cell per dimension")
        g = tuple(ghost if d < nd else 0 for d in range(3))
        du = tuple(1 if d < nd else 0 for d in range(3))
        pl, pr = [0, 0, 0], [0, 0, 0]
        if align:
            pl[0] = (align - g[0] % align) % align
            tot = pl[0] + g[0] + du[0] + inner[0] + du[0] + g[0]
            pr[0] = (align - tot % align) % align
        return FieldLayout(nd, inner, g, du, tuple(pl), tuple(pr), communicates_dup, communicates_ghost)

    # -- sizes ---------------------------------------------------------------------------------
    def tot(self, d: int) -> int:
        return self.pad_l[d] + self.ghost[d] + self.dup[d] + self.inner[d] + self.dup[d] + self.ghost[d] + self.pad_r[d]

    def ref(self, d: int) -> int:
        return self.pad_l[d] + self.ghost[d]

    @property
    def size(self) -> int:
        if self.transform == 1:
            return 2 * ((self.tot(0) + 1) // 2) * self.tot(1) * self.tot(2)
        return self.tot(0) * self.tot(1) * self.tot(2)

    def split_x(self) -> "FieldLayout":
        """This layout under the colour split `[x, y, z] => [x / 2, y, z, x % 2]`."""
        from dataclasses import replace

        return replace(self, transform=1)

    def plain(self) -> "FieldLayout":
        from dataclasses import replace

        return replace(self, transform=0)

    def linear(self, i0: int, i1: int = 0, i2: int = 0) -> int:
        """Array index of iterator point (i0, i1, i2) -- the restatement of the library's index map (csrc/examg_common.h: lidx)."""
        a = (i0 + self.ref(0), i1 + self.ref(1), i2 + self.ref(2))
        if self.transform == 1:
            hx = (self.tot(0) + 1) // 2
            return a[0] // 2 + hx * (a[1] + self.tot(1) * (a[2] + self.tot(2) * (a[0] % 2)))
        return a[0] + self.tot(0) * (a[1] + self.tot(1) * a[2])

    @property
    def shape_zyx(self) -> Tuple[int, int, int]:
        return (self.tot(2), self.tot(1), self.tot(0))

    # -- region markers in iterator coordinates (IR_FieldLayout.defIdxById minus referenceOffset) --
    def idx(self, name: str, d: int) -> int:
        g, du, n = self.ghost[d], self.dup[d], self.inner[d]
        table = {
            "GLB": -g, "GLE": 0, "DLB": 0, "DLE": du, "IB": du, "IE": du + n,
            "DRB": du + n, "DRE": 2 * du + n, "GRB": 2 * du + n, "GRE": 2 * du + n + g,
        }
        return table[name]

    def dup_plane(self, d: int, side: int):
        """Box of the duplicate plane at face (d, side), tangentially DLB..DRE: where a physical face holds its boundary values."""
        pb = [self.idx("DLB", t) if t < self.nd else 0 for t in range(3)]
        pe = [self.idx("DRE", t) if t < self.nd else 1 for t in range(3)]
        pb[d], pe[d] = (self.idx("DLB", d), self.idx("DLE", d)) if side < 0 else (self.idx("DRB", d), self.idx("DRE", d))
        return pb, pe

    def c_struct(self) -> LayoutC:
        s = LayoutC()
        s.nd = self.nd
        for d in range(3):
            s.pad_l[d], s.pad_r[d] = self.pad_l[d], self.pad_r[d]
            s.ghost_l[d] = s.ghost_r[d] = self.ghost[d]
            s.dup_l[d] = s.dup_r[d] = self.dup[d]
            s.inner[d] = self.inner[d]
        s.transform = self.transform
        return s
