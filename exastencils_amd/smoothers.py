"""Temporally blocked smoother steps (two Jacobi steps per pass over HBM), also across block neighbours.

Reference idea: `repeat n times with contraction` / IR_ContractingLoop (Compiler/src/exastencils/baseExt/ir/
IR_ContractingLoop.scala; Testing/PolyExpl/Jac3Dcc.exa4:27) and the `Comm*TempBlockable` layouts of the
generated-from-L3 programs.  The reference widens the ghost layers to block in time; here the ghost layers stay
one deep (the drop-in layout) and the block is split into a deep interior, which needs no halo at all for two steps,
and a two-point shell along the interior faces:

  main stream   u_out = J(J(u)) on the loop's box shrunk by 2 at interior faces; the first step is evaluated on the box
                shrunk by 1 (examg_jacobi2_boxes) -- reads no ghost value, starts immediately
  side stream   1. communicate ghost of u                      (as every Smoother call does)
                2. tmp = J(u) on the three planes next to every interior face       (thin launches)
                3. communicate ghost of tmp                    (the neighbours' first-step values)
                4. u_out = J(tmp) on the two planes next to every interior face     (thin launches)
  join          (events)

Two exchanges per two steps -- as many as two plain Smoother calls -- all of it (pack, RCCL send/recv over xGMI, unpack,
thin kernels) overlapped with the one large kernel, and bit-identical results.  This is the reference's core/boundary
split (Compiler/src/exastencils/baseExt/ir/IR_LoopOverPointsInOneFragment.scala:143-222,
experimental_splitLoopsForAsyncComm) applied to a pair of steps.  On a single block only the main-stream launch remains.
"""
from __future__ import annotations

from .domain import shrink, slab

SMOOTH = 2


def beside(ops, side_fn, main_fn, overlap: bool = True, sequential: str = "side_first"):
    """`side_fn()` on the kernel layer's side stream beside `main_fn()` on the current one: the side stream first waits for everything
    issued so far, the current stream afterwards for the side stream.  Without a side stream (CPU kernel layer) or without `overlap` the
    two run one after the other, in the order `sequential` names ("side_first" | "main_first")."""
    if not (overlap and hasattr(ops, "side_stream")):
        for fn in (side_fn, main_fn) if sequential == "side_first" else (main_fn, side_fn):
            fn()
        return
    torch, side = ops.torch, ops.side_stream()
    main = torch.cuda.current_stream(ops.device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        side_fn()
    main_fn()
    main.wait_stream(side)


def deep_halo_boxes(ops, domain, S, F, A, b, e, faces):
    """Temporal blocking across block neighbours by DEEPER HALOS instead of a recomputed shell -- the reference's own way
    (baseExt/ir/IR_ContractingLoop.scala:45-196 on a layout with `ghostLayers` >= 2): with two exchanged ghost layers of the input (and
    one of the right-hand side) the first stage runs on the loop's box grown by one point across every interior face -- the neighbour's
    first plane is computed here too, from the same bits with the same kernel -- and the second stage on the loop's own box: ONE exchange
    and ONE kernel per pass, no scratch field, nothing beside the kernel that competes with it.  Returns the first-stage box, or None
    when the layouts have no room for it (then the shell scheme below runs)."""
    lay, flay = S.layout, F.layout
    if not faces or any(lay.ghost[d] < 2 or flay.ghost[d] < 1 for d, _ in faces) or not (lay.communicates_ghost and flay.communicates_ghost):
        return None
    b1, e1 = shrink(b, e, faces, -1)
    if hasattr(ops, "two_stage_eligible") and not ops.two_stage_eligible(S.lc, F.lc, A, b1, e1, list(b), list(e)):
        return None
    return b1, e1


def _edges_matter(faces) -> bool:
    """More than one axis with neighbours: the first stage on a ghost plane reads edge ghosts, which only the axis-by-axis exchange fills."""
    return len({d for d, _ in faces}) > 1


def jacobi_triple(ops, comm, domain, S, F, A, w: float, tmp_field) -> bool:
    """Three applications of `Smoother@current` on field S (2 slots) in ONE pass (examg_jacobi3: temporal blocking of depth 3), on a block
    without neighbours: reads slot <active>, writes the other slot, one advance -- the slot three advances make active.  Returns False
    (nothing done) on a block with neighbours: three steps without an exchange would need three ghost layers; the caller runs a pair and
    a step there."""
    if domain.interior_faces():
        return False
    b, e = domain.loop_bounds(S.layout)
    if hasattr(ops, "three_stage_eligible") and not ops.three_stage_eligible(S.lc, F.lc, A, list(b), list(e)):
        return False        # the entry point would run a step through `tmp` (with a copy of the box) and a pair: the caller's pair + step is cheaper
    comm.exchange(S, S.active, "ghost", A.faces_only)      # empty on a single block
    ops.jacobi3(S.lc, S.data(S.active), S.data(S.next), tmp_field.data(), F.lc, F.data(), A, w, b, e)
    S.advance()
    return True


def _two_stage_pass(kind: str, ops, comm, domain, S, F, A, w: float, tmp_field, *, overlap: bool, u_out, lone, slot=None, first: int = 0,
                    copy_planes: bool = True):
    """Two dependent loops over S's box -- two Jacobi steps (kind "jacobi2") or the two colours of a red-black sweep that starts with
    colour `first` (kind "rbgs") -- from S's slot `slot` (None: the active one) into array u_out as one pass, by the first route that
    applies:

      1. no neighbours: `lone(b, e)`, the caller's one-pass call on the whole box
      2. deep halos (deep_halo_boxes): one exchange, one kernel on the grown box
      3. the communicator's library call (comm.c_pass; csrc/examg_comm.hip: pass_blocks), which is 4. and 5. in C -- the Python form
         that follows is the same sequence statement by statement; it serves the CPU kernel layer (gloo tests) and is what the library
         call is tested against (tests/test_gpu_transport.py)
      4. deep interior (box shrunk by one point at interior faces for the first loop, by two for the second) + two-point shell: exchange S,
         first loop on three planes per interior face into tmp, exchange tmp, second loop on two planes into u_out
      5. ... the shell on the side stream beside the interior where the kernel layer runs the interior as one kernel
         (examg_two_stage_eligible, the route function the entry point itself switches on -- stencil kind AND entry order, row length, box
         inside the allocation), else interior first: the fallback of the two-box entry points (short rows on coarse levels, other
         stencils) uses tmp as scratch for its whole first loop and must finish before the shell work writes tmp.

    A red-black slab starts as a copy of its input and has the colour's points updated; a Jacobi slab is launched straight from its
    input.  The caller makes u_out current."""
    assert kind in ("jacobi2", "rbgs")
    jacobi = kind == "jacobi2"
    colours = (-1, -1) if jacobi else (first, 1 - first)
    u_in = S.data(slot)
    b, e = domain.loop_bounds(S.layout)
    faces = domain.interior_faces()
    axis_only = A.faces_only                     # 5/7-point: face ghosts suffice
    tmp = tmp_field.data()
    probe = hasattr(ops, "two_stage_eligible")

    def boxes(scratch, b1, e1, b2, e2):
        if jacobi:                                   # always through tmp: the entry point takes no other scratch
            ops.jacobi2_boxes(S.lc, u_in, u_out, tmp, F.lc, F.data(), A, w, b1, e1, b2, e2)
        else:
            ops.rbgs_sweep_fused_boxes(S.lc, u_in, u_out, scratch, F.lc, F.data(), A, w, first, b1, e1, b2, e2)

    if not faces:
        comm.exchange(S, slot, "ghost", axis_only)      # empty on a single block
        lone(b, e)
        return
    deep = deep_halo_boxes(ops, domain, S, F, A, b, e, faces)
    if deep is not None:
        comm.exchange(S, slot, "ghost", axis_only and not _edges_matter(faces))
        boxes(None if probe else tmp, deep[0], deep[1], list(b), list(e))      # the CPU kernel layer runs the two loops through a copy
        return
    if hasattr(comm, "c_pass") and comm.c_pass(kind, S, u_in, u_out, tmp, F, A, w, first, b, e, axis_only, overlap,
                                               not copy_planes):
        return
    b1, e1 = shrink(b, e, faces, 1)
    b2, e2 = shrink(b, e, faces, 2)
    has_interior = all(e2[d] > b2[d] for d in range(domain.nd))
    fused = probe and has_interior and ops.two_stage_eligible(S.lc, F.lc, A, b1, e1, b2, e2)
    concurrent = overlap and fused and hasattr(ops, "side_stream")

    def interior():
        if has_interior:
            boxes(None if concurrent else tmp, b1, e1, b2, e2)

    def slabs(k, u, out, colour):
        for d, side in faces:
            sb, se = slab(b, e, d, side, k)
            if not jacobi:
                ops.axpby(S.lc, u, S.lc, out, 1.0, 0.0, sb, se)
            ops.stencil_op(SMOOTH, S.lc, u, F.lc, F.data(), S.lc, out, A, w, colour, sb, se)

    def shell():
        comm.exchange(S, slot, "ghost", axis_only)
        # tmp's duplicate planes on PHYSICAL faces are read by the second loop of the slabs (tangential neighbours) and written by
        # nobody: bring them over from the input, whatever boundary values the program put there (Dirichlet function, or SetFuncDir
        # values during an FMG start) -- unless the caller wrote them once (position-only values)
        for d, side in domain.physical_faces() if copy_planes else ():
            ops.axpby(S.lc, u_in, S.lc, tmp, 1.0, 0.0, *S.layout.dup_plane(d, side))
        slabs(3, u_in, tmp, colours[0])
        comm.exchange(tmp_field, None, "ghost", axis_only)
        slabs(2, tmp, u_out, colours[1])

    beside(ops, shell, interior, concurrent, sequential="main_first")


def jacobi_pair(ops, comm, domain, S, F, A, w: float, tmp_field, overlap: bool = True, correction_from=None):
    """Two applications of `Smoother@current` (Testing/Smoothers/Jac.exa4:125-131) on field S (2 slots):
    reads slot <active>, leaves the result in the slot two `advance`s would make active (the same one),
    reached through one advance of the out-of-place pass.  tmp_field: scratch field of S's layout whose
    Dirichlet shell holds S's boundary values.  correction_from (single block only): the coarser Solution field whose
    prolongation `Correction@current` adds to S just before the pair -- folded into the pass (examg_jacobi2_prolong)."""
    u_in, u_out, Sc = S.data(S.active), S.data(S.next), correction_from
    assert Sc is None or not domain.interior_faces(), "the folded correction needs a block without neighbours"

    def lone(b, e):
        if Sc is not None:
            ops.jacobi2_prolong(S.lc, u_in, u_out, tmp_field.data(), F.lc, F.data(), A, w, b, e, Sc.lc, Sc.data())
        else:
            ops.jacobi2_boxes(S.lc, u_in, u_out, tmp_field.data(), F.lc, F.data(), A, w, b, e, b, e)

    _two_stage_pass("jacobi2", ops, comm, domain, S, F, A, w, tmp_field, overlap=overlap, slot=S.active, u_out=u_out, lone=lone)
    S.advance()


def rbgs_sweep(ops, comm, domain, S, F, A, w: float, alt, tmp_field, first: int = 0, overlap: bool = True, tmp_planes_valid: bool = False):
    """One red-black sweep of `repeat { color with { (i0+i1+i2) % 2, communicate S; loop over S { S += w (F - A S) };
    apply bc to S } }` (Benchmark/Poisson3D/3D_FD_Poisson_fromL4.exa4:204-213), out of place from S's array into `alt`; returns the
    array that is free afterwards (S's former one) -- the two change roles.

    With neighbours (_two_stage_pass): both arrays and tmp carry S's Dirichlet values on the physical faces (tmp_planes_valid: the
    caller wrote tmp's once, `apply bc` values are position-only); results are bit-identical to the two in-place half sweeps."""
    src = S.data()
    _two_stage_pass("rbgs", ops, comm, domain, S, F, A, w, tmp_field, overlap=overlap, u_out=alt, first=first, copy_planes=not tmp_planes_valid,
                    lone=lambda b, e: ops.rbgs_sweep_fused(S.lc, src, alt, F.lc, F.data(), A, w, first, b, e))
    S.slots[S.active] = alt
    return src


def overlapped_loop(ops, domain, b, e, exchange_ghost, kernel, overlap: bool = True):
    """`communicate ghost of f; loop over g { ... reads f within one point ... }` on a block with neighbours, as the
    reference's core/boundary split does it (Compiler/src/exastencils/baseExt/ir/IR_LoopOverPointsInOneFragment.scala:143-222,
    experimental_splitLoopsForAsyncComm): the loop's box shrunk by one point at every interior face reads no ghost value
    and starts at once; the exchange (pack, RCCL send / recv, unpack) runs on the side stream meanwhile; the one-point
    shell -- disjoint slabs, so that accumulating loops (`+=`) stay correct -- follows when the halo is in.  Used for
    the residual (reads Solution's ghosts) and for the restriction (its coarse box shrunk by one point reads no fine ghost).
    `kernel(begin, end)` launches the loop on a sub-box; same bits as exchange + one launch over [b, e)."""
    faces = domain.interior_faces()
    ib, ie = shrink(b, e, faces, 1)
    if not faces or any(ie[d] - ib[d] < 1 for d in range(domain.nd)):      # no neighbours, or a block too thin to have an interior: plain order
        exchange_ghost()
        kernel(b, e)
        return
    beside(ops, exchange_ghost, lambda: kernel(ib, ie), overlap, sequential="side_first")
    lo, hi = list(b), list(e)
    for d in range(domain.nd):
        for side in (-1, 1):
            if (d, side) in faces:
                kernel(*slab(lo, hi, d, side, 1))
        lo[d], hi[d] = ib[d], ie[d]            # the slabs of the axes that follow leave out what these covered
