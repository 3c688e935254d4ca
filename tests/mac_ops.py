"""TEST-ONLY restatement of the staggered-grid entry points (include/examg.h: examg_mac_op, examg_mac_relax, examg_mac_sweep,
examg_restrict_face, examg_prolong_add_face, examg_apply_bc_face, examg_fill_expr_face, examg_max_err_expr_face) in numpy, on top of the
cell oracle layer (tests/cell_ops.py).  Every operation in the order the header fixes, one IEEE double operation at a time (numpy does
not contract); the cells of a colour are strided slices.  The refusals are restated too, so that the CPU suite sees them."""
import itertools

import numpy as np

from cell_ops import CellOracleOps, _empty

SYS_APPLY, SYS_RESIDUAL = 0, 1
BC_DIRICHLET, BC_NEUMANN = 0, 1


class MacError(RuntimeError):
    pass


def _cs(l):
    return l.c_struct() if hasattr(l, "c_struct") else l


def _view(l, x):
    """x as a (z, y, x) array, and the reference offsets."""
    l = _cs(l)
    ref = [l.pad_l[d] + l.ghost_l[d] for d in range(3)]
    tot = [l.pad_l[d] + l.ghost_l[d] + l.dup_l[d] + l.inner[d] + l.dup_r[d] + l.ghost_r[d] + l.pad_r[d] for d in range(3)]
    return x.numpy().reshape(tot[2], tot[1], tot[0]), ref, tot


def _pts(v, b, e, off=(0, 0, 0), step=(1, 1, 1)):
    """View of the points b, b + step, .. < e displaced by `off` (x, y, z)."""
    a, ref = v[0], v[1]
    return a[tuple(slice(b[d] + off[d] + ref[d], e[d] + off[d] + ref[d], step[d]) for d in (2, 1, 0))]


def _inside(v, b, e, lo=(0, 0, 0), hi=(0, 0, 0)):
    ref, tot = v[1], v[2]
    return all(e[d] <= b[d] or (b[d] - lo[d] + ref[d] >= 0 and e[d] + hi[d] + ref[d] <= tot[d]) for d in range(3))


def _e(d, s=1):
    o = [0, 0, 0]
    o[d] = s
    return tuple(o)


def _fold(st, v, b, e, step, skip, about=(0, 0, 0)):
    """The entries of `st` that are not in `skip`, folded left to right in declared order about the points displaced by `about`."""
    acc = None
    for o, c in zip(st.offsets, st.coefs):
        if tuple(o) in skip:
            continue
        t = float(c) * _pts(v, b, e, tuple(o[k] + about[k] for k in range(3)), step)
        acc = t if acc is None else acc + t
    return acc


def _coef(st, off):
    offs = [tuple(o) for o in st.offsets]
    return float(st.coefs[offs.index(off)]) if off in offs else 0.0


def _layout_pattern(who, what, l, nd, loc, n):
    l = _cs(l)
    if l.nd != nd:
        raise MacError("%s: the %s layout has %d dimensions, the system %d" % (who, what, l.nd, nd))
    if l.transform:
        raise MacError("%s: the %s layout is under a layout transformation; staggered fields take plain layouts only" % (who, what))
    for d in range(nd):
        dup = 1 if d == loc else 0
        if l.dup_l[d] != dup or l.dup_r[d] != dup:
            if loc < 0:
                raise MacError("%s: the %s layout is not a cell layout (dim %d has %d / %d duplicate layers)" % (who, what, d, l.dup_l[d], l.dup_r[d]))
            raise MacError("%s: the %s layout is not a face layout of axis %d (dim %d has %d / %d duplicate layers, a face layout has %d)"
                           % (who, what, loc, d, l.dup_l[d], l.dup_r[d], dup))
        cells = l.inner[d] + dup
        if cells < 1:
            raise MacError("%s: the %s layout has no cell in dim %d" % (who, what, d))
        if n[d] == 0:
            n[d] = cells
        if cells != n[d]:
            raise MacError("%s: the %s layout has %d cells in dim %d, the pressure %d" % (who, what, cells, d, n[d]))


def _ghost(who, what, l):
    l = _cs(l)
    for d in range(l.nd):
        if l.ghost_l[d] < 1 or l.ghost_r[d] < 1:
            raise MacError("%s: %s has no ghost layer in dim %d" % (who, what, d))


def check_system(who, sys, relax, need_f, rows):
    """The checks of mac_prepare (csrc/kernels_mac.hip), in its order.  Returns the cells per axis."""
    sys.check_elements(who)
    nd = sys.nd
    if nd not in (2, 3):
        raise MacError("%s: nd = %d; staggered systems are 2-D or 3-D" % (who, nd))
    n = [0, 0, 0]
    _layout_pattern(who, "pressure", sys.lp, nd, -1, n)
    _ghost(who, "the pressure", sys.lp)
    for d in range(nd):
        _layout_pattern(who, "u_%d" % d, sys.lu[d], nd, d, n)
        _ghost(who, "u_%d" % d, sys.lu[d])
    unknowns = list(sys.u[:nd]) + [sys.p]
    fs = (list(sys.f[:nd]) if sys.f else [None] * nd) + [sys.fp]
    lfs = (list(sys.lf[:nd]) if sys.lf else [None] * nd) + [sys.lfp]
    dsts = (list(sys.dst[:nd]) if sys.dst else [None] * nd) + [sys.dstp]
    lds = (list(sys.ld[:nd]) if sys.ld else [None] * nd) + [sys.ldp]
    for r in range(nd + 1):
        if not (rows >> r) & 1:
            continue
        loc = r if r < nd else -1
        if need_f:
            if fs[r] is None:
                raise MacError("%s: right-hand side %d is a null pointer" % (who, r))
            _layout_pattern(who, "rhs %d" % r, lfs[r], nd, loc, n)
        if not relax:
            if dsts[r] is None:
                raise MacError("%s: destination %d is a null pointer" % (who, r))
            _layout_pattern(who, "dst %d" % r, lds[r], nd, loc, n)
            for c in range(nd + 1):
                if dsts[r] is unknowns[c]:
                    raise MacError("%s: destination %d is unknown %d; the operator does not run in place" % (who, r, c))
                if need_f and (rows >> c) & 1 and dsts[r] is fs[c]:
                    raise MacError("%s: destination %d is right-hand side %d; the rows are evaluated side by side" % (who, r, c))
                if c != r and (rows >> c) & 1 and dsts[r] is dsts[c]:
                    raise MacError("%s: destinations %d and %d are one array" % (who, r, c))
    for d in range(nd):
        st = sys.A[d]
        if st is None:
            raise MacError("%s: A_%d is a null pointer" % (who, d))
        if st.cfield is not None:
            raise MacError("%s: A_%d is a stencil field; the velocity blocks are constant stencils" % (who, d))
        if not 1 <= len(st.offsets) <= 7:
            raise MacError("%s: A_%d: nent %d outside 1 .. 7" % (who, d, len(st.offsets)))
        seen = set()
        for k, o in enumerate(st.offsets):
            nz = [t for t in range(3) if o[t]]
            if len(nz) > 1 or (nz and (nz[0] >= nd or abs(o[nz[0]]) > 1)):
                raise MacError("%s: A_%d, entry %d (%d, %d, %d) is not the centre or an axis neighbour at distance 1 of a %d-D field"
                               % (who, d, k, o[0], o[1], o[2], nd))
            if tuple(o) in seen:
                raise MacError("%s: A_%d, entry %d repeats the offset (%d, %d, %d)" % (who, d, k, o[0], o[1], o[2]))
            seen.add(tuple(o))
        if (0, 0, 0) not in seen:
            raise MacError("%s: A_%d has no centre entry" % (who, d))
    return n


def check_colouring(who, col, nd, with_rem=True):
    if not 1 <= len(col.exprs) <= 3:
        raise MacError("%s: colouring: nexpr must be 1, 2 or 3" % who)
    for axes, shift, mod in col.exprs:
        if mod <= 0:
            raise MacError("%s: colouring: mod must be positive" % who)
        if not axes or any(d >= nd for d in axes):
            raise MacError("%s: colouring: axes must name a non-empty set of the layout's axes" % who)
    near = lambda r: itertools.product(range(-r, r + 1), range(-r, r + 1), range(-r, r + 1) if nd == 3 else (0,))
    for o in itertools.chain(near(1), near(2)):      # the neighbours first: the conflict named is the nearest one
        if 1 <= sum(abs(t) for t in o) <= 2 and not col.decouples([o]):
            raise MacError("%s: the colouring does not decouple the boxes: cells i and i + (%d, %d, %d) have the same colour, and the box of one "
                           "reads or writes a face or a pressure of the other's -- an in-place loop over one colour would depend on the loop order"
                           % (who, o[0], o[1], o[2]))
    axes_seen = set()
    for axes, shift, mod in col.exprs:
        if len(axes) != 1 or axes[0] in axes_seen or mod < 3:
            raise MacError("%s: colouring: the box smoother takes one expression (s_d + i_d) %% m_d per axis, every m_d >= 3" % who)
        axes_seen.add(axes[0])
    if len(col.exprs) != nd:
        raise MacError("%s: colouring: the box smoother takes one expression (s_d + i_d) %% m_d per axis, every m_d >= 3" % who)


def _block(sys, d, h0, h1):
    """The 2 x 2 block, its border column of axis d under the hold pattern; arrays or scalars."""
    st = sys.A[d]
    a, q, m = _coef(st, (0, 0, 0)), _coef(st, _e(d, 1)), _coef(st, _e(d, -1))
    w = np.where
    return (w(h0, 1.0, a), w(h0, 0.0, q), w(h1, 0.0, m), w(h1, 1.0, a), w(h0, 0.0, float(sys.bc[d])), w(h1, 0.0, float(sys.bm[d])))


def check_regular(who, sys, n):
    nd = sys.nd
    states = []
    for d in range(nd):
        states.append([3] if n[d] == 1 else ([1, 2] + ([0] if n[d] > 2 else [])))
    for st in itertools.product(*states):
        sz = None
        for d in range(nd):
            a00, a01, a10, a11, c0, c1 = [float(v) for v in _block(sys, d, bool(st[d] & 1), bool(st[d] & 2))]
            det = a00 * a11 - a01 * a10
            if det == 0.0:
                raise MacError("%s: the 2 x 2 block of the faces of axis %d has the determinant zero" % (who, d))
            z0, z1 = (c0 * a11 - a01 * c1) / det, (a00 * c1 - a10 * c0) / det
            tz = float(sys.cc[d]) * z0
            sz = tz if sz is None else sz + tz
            sz = sz + float(sys.cp[d]) * z1
        if sz == 0.0:
            raise MacError("%s: the Schur complement of a cell's pressure is zero (held faces per axis: %s; 3 = both: fewer than 2 cells on every axis?)"
                           % (who, ", ".join(str(s) for s in st)))


def face_positions(axis, geom, b, e):
    """The positions of the faces of `axis` in the box: the node position on the own axis, the cell centre on the others."""
    i2, i1, i0 = np.meshgrid(np.arange(b[2], e[2]), np.arange(b[1], e[1]), np.arange(b[0], e[0]), indexing="ij")
    out = []
    for d, i in enumerate((i0, i1, i2)):
        p = i * geom.h[d] + geom.pos_begin[d]
        out.append(p if d == axis else p + 0.5 * geom.h[d])
    return out


def _face_layout(who, what, axis, l):
    l = _cs(l)
    if l.nd not in (2, 3):
        raise MacError("%s: 2-D or 3-D layouts" % who)
    if not 0 <= axis < l.nd:
        raise MacError("%s: axis %d of a %d-D face field" % (who, axis, l.nd))
    n = [0, 0, 0]
    _layout_pattern(who, what, l, l.nd, axis, n)
    return n


class MacOracleOps(CellOracleOps):
    name = "mac-oracle"

    # -- the operator -----------------------------------------------------------------------------------------------------
    def mac_op(self, mode, sys, row_mask, begin, end):
        who = "examg_mac_op"
        if mode not in (SYS_APPLY, SYS_RESIDUAL):
            raise MacError("%s: bad mode %d" % (who, mode))
        if sys.nd not in (2, 3):
            raise MacError("%s: nd = %d; staggered systems are 2-D or 3-D" % (who, sys.nd))
        nd = sys.nd
        if row_mask == 0 or row_mask >> (nd + 1):
            raise MacError("%s: row mask 0x%x for %d rows" % (who, row_mask, nd + 1))
        check_system(who, sys, False, mode == SYS_RESIDUAL, row_mask)
        vu = [_view(sys.lu[d], sys.u[d]) for d in range(nd)]
        vp = _view(sys.lp, sys.p)
        out = []
        for r in range(nd + 1):
            if not (row_mask >> r) & 1:
                continue
            b, e = list(begin[r]), list(end[r])
            if _empty(b, e):
                continue
            if r < nd:
                st = sys.A[r]
                lo = [int(any(o[t] < 0 for o in st.offsets)) for t in range(3)]
                hi = [int(any(o[t] > 0 for o in st.offsets)) for t in range(3)]
                if not _inside(vu[r], b, e, lo, hi):
                    raise MacError("%s: row %d: box + the reach of A_%d leaves the allocation of u_%d" % (who, r, r, r))
                if not _inside(vp, b, e, _e(r), (0, 0, 0)):
                    raise MacError("%s: row %d: the gradient leaves the allocation of the pressure" % (who, r))
                conv = _fold(st, vu[r], b, e, (1, 1, 1), ())
                grad = (float(sys.bc[r]) * _pts(vp, b, e)) + (float(sys.bm[r]) * _pts(vp, b, e, _e(r, -1)))
                au = conv + grad
                vf = _view(sys.lf[r], sys.f[r]) if mode == SYS_RESIDUAL else None
                vd = _view(sys.ld[r], sys.dst[r])
            else:
                au = None
                for d in range(nd):
                    if not _inside(vu[d], b, e, (0, 0, 0), _e(d)):
                        raise MacError("%s: row %d: the divergence leaves the allocation of u_%d" % (who, r, d))
                    lo_ = float(sys.cc[d]) * _pts(vu[d], b, e)
                    hi_ = float(sys.cp[d]) * _pts(vu[d], b, e, _e(d))
                    au = lo_ if au is None else au + lo_
                    au = au + hi_
                vf = _view(sys.lfp, sys.fp) if mode == SYS_RESIDUAL else None
                vd = _view(sys.ldp, sys.dstp)
            if vf is not None and not _inside(vf, b, e):
                raise MacError("%s: row %d: box leaves the rhs allocation" % (who, r))
            if not _inside(vd, b, e):
                raise MacError("%s: row %d: box leaves the dst allocation" % (who, r))
            out.append((vd, b, e, _pts(vf, b, e) - au if vf is not None else au))
        for vd, b, e, val in out:
            _pts(vd, b, e)[...] = val

    # -- the box smoother -------------------------------------------------------------------------------------------------
    def _relax_checks(self, who, sys, col, begin, end, with_rem):
        if sys.nd not in (2, 3):
            raise MacError("%s: nd = %d; staggered systems are 2-D or 3-D" % (who, sys.nd))
        nd = sys.nd
        n = check_system(who, sys, True, True, (1 << (nd + 1)) - 1)
        check_colouring(who, col, nd, with_rem)
        check_regular(who, sys, n)
        if _empty(begin, end):
            return None
        for d in range(nd):
            if begin[d] < 0 or end[d] > n[d]:
                raise MacError("%s: the box [%d, %d) of dim %d leaves the cells [0, %d) of the block" % (who, begin[d], end[d], d, n[d]))
        for d in range(nd):
            if not _inside(_view(sys.lf[d], sys.f[d]), begin, end, (0, 0, 0), _e(d)):
                raise MacError("%s: box leaves the allocation of rhs %d" % (who, d))
        if not _inside(_view(sys.lfp, sys.fp), begin, end):
            raise MacError("%s: box leaves the allocation of rhs %d" % (who, nd))
        for axes, shift, mod in col.exprs:
            if shift + sum(begin[d] for d in axes) < 0:
                raise MacError("%s: a colour expression can be negative in this box (shift + begin < 0)" % who)
        return n

    def mac_relax(self, sys, relax, col, begin, end, cells=None):
        """cells: test hook -- restrict the colour to these cells, visited one at a time in the given order (the decoupling claim says
        the order does not matter)."""
        n = self._relax_checks("examg_mac_relax", sys, col, begin, end, True)
        if n is None:
            return
        first, step = list(begin), [1, 1, 1]
        for (axes, shift, mod), rem in zip(col.exprs, col.rem):
            d = axes[0]
            step[d], first[d] = mod, begin[d] + (rem - (shift + begin[d])) % mod
        if _empty(first, end):
            return
        if cells is not None:
            for c in cells:
                self._solve(sys, relax, list(c), [c[0] + 1, c[1] + 1, c[2] + 1], [1, 1, 1], n)
            return
        self._solve(sys, relax, first, list(end), step, n)

    def _solve(self, sys, relax, b, e, step, n):
        nd = sys.nd
        vu = [_view(sys.lu[d], sys.u[d]) for d in range(nd)]
        vf = [_view(sys.lf[d], sys.f[d]) for d in range(nd)]
        vp, vfp = _view(sys.lp, sys.p), _view(sys.lfp, sys.fp)
        idx = np.meshgrid(np.arange(b[2], e[2], step[2]), np.arange(b[1], e[1], step[1]), np.arange(b[0], e[0], step[0]), indexing="ij")[::-1]
        ys, zs, holds, sy, sz = [], [], [], None, None
        with np.errstate(all="ignore"):
            for d in range(nd):
                st = sys.A[d]
                tail_l = float(sys.bm[d]) * _pts(vp, b, e, _e(d, -1), step)
                tail_h = float(sys.bc[d]) * _pts(vp, b, e, _e(d, 1), step)
                fl = _fold(st, vu[d], b, e, step, {(0, 0, 0), _e(d, 1)})
                fh = _fold(st, vu[d], b, e, step, {(0, 0, 0), _e(d, -1)}, about=_e(d))
                tl = tail_l if fl is None else fl + tail_l
                th = tail_h if fh is None else fh + tail_h
                rl = _pts(vf[d], b, e, (0, 0, 0), step) - tl
                rh = _pts(vf[d], b, e, _e(d), step) - th
                old0, old1 = _pts(vu[d], b, e, (0, 0, 0), step).copy(), _pts(vu[d], b, e, _e(d), step).copy()
                h0, h1 = idx[d] == 0, idx[d] + 1 == n[d]
                a00, a01, a10, a11, c0, c1 = _block(sys, d, h0, h1)
                r0, r1 = np.where(h0, old0, rl), np.where(h1, old1, rh)
                det = a00 * a11 - a01 * a10
                y0, y1 = (r0 * a11 - a01 * r1) / det, (a00 * r1 - a10 * r0) / det
                z0, z1 = (c0 * a11 - a01 * c1) / det, (a00 * c1 - a10 * c0) / det
                ty, tz = float(sys.cc[d]) * y0, float(sys.cc[d]) * z0
                sy = ty if sy is None else sy + ty
                sz = tz if sz is None else sz + tz
                sy = sy + float(sys.cp[d]) * y1
                sz = sz + float(sys.cp[d]) * z1
                ys.append((y0, y1))
                zs.append((z0, z1))
                holds.append((h0, h1, old0, old1))
            pn = (sy - _pts(vfp, b, e, (0, 0, 0), step)) / sz
            for d in range(nd):
                h0, h1, old0, old1 = holds[d]
                x0, x1 = ys[d][0] - zs[d][0] * pn, ys[d][1] - zs[d][1] * pn
                if relax != 1.0:
                    x0, x1 = old0 + float(relax) * (x0 - old0), old1 + float(relax) * (x1 - old1)
                lo, hi = _pts(vu[d], b, e, (0, 0, 0), step), _pts(vu[d], b, e, _e(d), step)
                lo[...] = np.where(h0, old0, x0)
                hi[...] = np.where(h1, old1, x1)
            pv = _pts(vp, b, e, (0, 0, 0), step)
            pv[...] = pn if relax == 1.0 else pv + float(relax) * (pn - pv)

    def mac_sweep(self, sys, relax, col, begin, end):
        if self._relax_checks("examg_mac_sweep", sys, col, begin, end, False) is None:
            return
        for c in col.colours():
            self.mac_relax(sys, relax, c, begin, end)

    # -- transfers of a face field ------------------------------------------------------------------------------------------
    def _transfer_checks(self, who, axis, lfine, a, lc, c, begin, end):
        if _cs(lfine).nd != _cs(lc).nd:
            raise MacError("%s: layouts of one dimensionality" % who)
        _face_layout(who, "fine", axis, lfine)
        _face_layout(who, "coarse", axis, lc)
        if a is c:
            raise MacError("%s: the two arrays are one" % who)

    def restrict_face(self, axis, lfine, rf, lc, fc, scale, begin, end):
        who = "examg_restrict_face"
        self._transfer_checks(who, axis, lfine, rf, lc, fc, begin, end)
        if _empty(begin, end):
            return
        nd = _cs(lfine).nd
        vf, vc = _view(lfine, rf), _view(lc, fc)
        fb = [(2 * begin[d] - 1 if d == axis else 2 * begin[d]) if d < nd else 0 for d in range(3)]
        fe = [(2 * (end[d] - 1) + 2 if d == axis else 2 * end[d]) if d < nd else 1 for d in range(3)]
        if not _inside(vc, begin, end) or not _inside(vf, fb, fe):
            raise MacError("%s: box leaves an allocation" % who)
        half = 0.25 if nd == 3 else 0.5
        w = {-1: scale * (0.25 * half), 0: scale * (0.5 * half), 1: scale * (0.25 * half)}
        ranges = [((-1, 0, 1) if d == axis else (0, 1)) if d < nd else (0,) for d in range(3)]
        acc = None
        for o in itertools.product(*ranges):      # x outermost, then y, then z
            sl = tuple(slice(2 * begin[d] + o[d] + vf[1][d], 2 * (end[d] - 1) + o[d] + vf[1][d] + 1, 2) if d < nd else
                       slice(begin[d] + vf[1][d], end[d] + vf[1][d]) for d in (2, 1, 0))
            t = w[o[axis]] * vf[0][sl]
            acc = t if acc is None else acc + t
        _pts(vc, begin, end)[...] = acc

    def prolong_add_face(self, axis, lc, uc, lfine, uf, begin, end):
        who = "examg_prolong_add_face"
        self._transfer_checks(who, axis, lfine, uf, lc, uc, begin, end)
        if _empty(begin, end):
            return
        nd = _cs(lfine).nd
        if begin[axis] < 0:
            raise MacError("%s: negative index on the field's own axis (the parity cases are those of a loop that starts at the boundary face 0)" % who)
        vf, vc = _view(lfine, uf), _view(lc, uc)
        cb = [begin[d] >> 1 if d < nd else 0 for d in range(3)]
        ce = [((end[d] >> 1) if d == axis else ((end[d] - 1) >> 1)) + 1 if d < nd else 1 for d in range(3)]
        if not _inside(vf, begin, end) or not _inside(vc, cb, ce):
            raise MacError("%s: box leaves an allocation" % who)
        i = [np.arange(begin[d], end[d]) for d in range(3)]

        def coarse(own):
            sel = [(own if d == axis else (i[d] >> 1 if d < nd else i[d])) + vc[1][d] for d in (2, 1, 0)]
            return vc[0][np.ix_(*sel)]

        own = i[axis]
        even = coarse(own >> 1)
        odd = (0.5 * coarse((own + 1) >> 1)) + (0.5 * coarse((own - 1) >> 1))
        shape = [1, 1, 1]
        shape[2 - axis] = own.size
        add = np.where((own & 1).reshape(shape) == 1, odd, even)
        s = _pts(vf, begin, end)
        s[...] = s + add

    # -- apply bc of a face field ---------------------------------------------------------------------------------------------
    def apply_bc_face(self, axis, l, x, geom, kind, expr, face_mask):
        who = "examg_apply_bc_face"
        if kind not in (BC_DIRICHLET, BC_NEUMANN):
            raise MacError("%s: kind %d; face fields take EXAMG_BC_DIRICHLET or EXAMG_BC_NEUMANN" % (who, kind))
        n = _face_layout(who, "field's", axis, l)
        lc_ = _cs(l)
        nd = lc_.nd
        if kind == BC_NEUMANN and face_mask & (3 << (2 * axis)):
            raise MacError("%s: a Neumann wall normal to the field's own axis %d (the node rule for it is not built)" % (who, axis))
        for d in range(nd):
            for side in (0, 1):
                if face_mask & (1 << (2 * d + side)) and d != axis and (lc_.ghost_r[d] if side else lc_.ghost_l[d]) < 1:
                    raise MacError("%s: wall %d of dim %d has no ghost layer" % (who, side, d))
        v = _view(l, x)
        ev = lambda p: self._eval_program(expr.program, *p)
        for d in [axis] + [t for t in range(nd) if t != axis]:      # the node rule first
            for side in (0, 1):
                if not face_mask & (1 << (2 * d + side)):
                    continue
                b, e = [0, 0, 0], [1, 1, 1]
                for t in range(nd):
                    e[t] = n[t] + 1 if t == axis else n[t]
                if side == 0:
                    e[d] = 1
                else:
                    b[d] = e[d] - 1
                p = face_positions(axis, geom, b, e)
                if d == axis:
                    _pts(v, b, e)[...] = ev(p)
                    continue
                interior = _pts(v, b, e).copy()      # the normal walls of the mask are written already
                ghost = _pts(v, b, e, _e(d, 1 if side else -1))
                if kind == BC_NEUMANN:
                    ghost[...] = interior
                    continue
                p[d] = np.full_like(p[d], (n[d] if side else 0) * geom.h[d] + geom.pos_begin[d])
                ghost[...] = (2.0 * ev(p)) - interior

    # -- expressions at the face positions --------------------------------------------------------------------------------------
    def fill_expr_face(self, axis, l, x, geom, expr, begin, end):
        _face_layout("examg_fill_expr_face", "field's", axis, l)
        if _empty(begin, end):
            return
        _pts(_view(l, x), begin, end)[...] = self._eval_program(expr.program, *face_positions(axis, geom, begin, end))

    def max_err_expr_face(self, axis, l, x, geom, expr, begin, end, out=None):
        _face_layout("examg_max_err_expr_face", "field's", axis, l)
        out = self.new_scalar() if out is None else out
        out[0] = 0.0
        if not _empty(begin, end):
            out[0] = float(np.max(np.abs(_pts(_view(l, x), begin, end) - self._eval_program(expr.program, *face_positions(axis, geom, begin, end)))))
        return out
