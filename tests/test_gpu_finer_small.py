"""The subgrid > 1 travel path (travel_finer_grid: csrc/fmm_exact_lds.hip or fmm_exact.hip, then
fmm_band_k.hip in mode 1 on the quantised fine view, then scale_kernel) against the CPU band model
of that path (oracle/band_model.c oband_travel_finer) and the heap oracle, both from the correctly
rounded build, on the small-shape matrix of tests/finer_cases.py: every material path at subgrid 3,
5 and 9, grids from 2 x 2 up, sources on corners, edges and next to them (the stage windows clipped
on one side, on four sides, one window and not the other), the HBM walk at subgrid 11 and 13, every
band and prefix parameter alone, every member count, batches and a reused arena, the subgrid-1
prefix over a whole grid, and the drop-in entry point.  Needs a GPU: pytest -m gpu.

Two bars, the project's own: BAR = 1e-9 for max |T - B| / B against the band model over ALL cells,
and EXACT = 1e-12 against the heap oracle on the exact region (the cells the heap-ordered prefix
made known: T sg <= 0.999 tstop in the model; every cell where the whole field lies inside the
prefix).  tests/test_oracle.py::test_finer_case_matrix_preconditions holds the model's side.  The
measured values go to the session's parity envelope under "finer_small/...", before anything is
asserted.

A third check, for what neither bar can see: on the exact region the field must equal the heap
oracle BIT FOR BIT.  DESIGN §3 states both walks bit-identical to the sequential walk, the final
scaling is one correctly rounded IEEE division on both sides, and the oracle build uses the device's
own correctly rounded functions, so nothing on that region may differ; a final multiplication by
1.0 / sg instead of the division is wrong by one ulp (1.1e-16) in a share of the cells, far below
EXACT, and is caught only here.

Measured on the MI355X when the file was written: every cell of every field of every group
bit-equal to the band model (rel_max 0, exact_frac 1.0: 47 model and shape cases with 375 fields and
7.6 M cells, 14 parameter cases, 23 HBM-walk fields, the member, batch and arena runs), the exact
region (646 k cells in the model and shape group) bit-equal to the heap oracle, exact_lds 0 and 1
bit-identical on 90 fields, the 54 subgrid-1 fields bit-equal to oracle.travel, exact_redo 0
everywhere; the bars stay where the project has them.  No device bug was found.  Libraries built
with one of these changes failed this file while the rest of the GPU suite passed: the band width
from mat_jump instead of mat_jump / sg (26 tests fail), tstop one node further out (40), the final
scaling a multiplication by 1.0 / sg (71, all on the bit-for-bit check), no float32 rounding of
vel_map in the fine view alone (9: the many_* cases).  What the matrix found lies
on the model's side (finer_cases.py): two inputs on which the band reformulation itself
misses the 1e-2 bar against the heap oracle at subgrid > 1, replaced and named there; and no small
case whose heap passes the LDS walk's 4095 entries, so the exact_redo path stays untested.

get_option("cdelta") answers for subgrid 1 only, so the band width at subgrid > 1 is restated in
finer_cases.band_cdelta (the jump density, which the context does report, divided by sg) and is
the only source of the width the model runs with: a device that used another width fails BAR.
"""
import contextlib

import numpy as np
import pytest

import finer_cases as FC

pytestmark = pytest.mark.gpu

BAR = 1e-9
EXACT = 1e-12


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def _context(shared, case):
    """The shared context for a case with the library's own options, a fresh one (options are kept
    per context; a band width once set stays set) for a case that sets any."""
    import _alifmm

    if not case.opts:
        yield shared
        return
    c = _alifmm.Context(0)
    try:
        for k, v in case.opts.items():
            c.set_option(k, v)
        yield c
    finally:
        c.close()


def _set_model(c, case):
    """Upload the case's model; the context's vmax.  What the context reports of the band's inputs
    equals what the model is run with (lib_options): the jump density behind the automatic width,
    r0, exact_r, r_far, far_sg."""
    veln, velpn, vm, sd = FC.model_arrays(case.model, case.nz, case.nx)
    c.set_model(veln, velpn, vm, sd, FC.TABLE, FC.TABLE, case.dnx, case.dnz, case.gox, case.goz)
    want = FC.lib_options(case)
    assert abs(c.get_option("mat_jump") - FC.BC.jump_density(veln, velpn, vm, sd)) <= 1e-15, case.name
    for k in ("r0", "exact_r", "r_far", "far_sg"):
        assert c.get_option(k) == want[k], (case.name, k, c.get_option(k), want[k])
    if "cdelta" in case.opts:
        assert c.get_option("cdelta") == case.opts["cdelta"]
    return c.get_option("vmax")


def _travel(c, case, srcs):
    xy = [FC.source_xy(case, s) for s in srcs]
    return c.travel([p[0] for p in xy], [p[1] for p in xy], subgrid=case.sg)


def _vs_refs(envelope, group, case, srcs, fields, vmax, whole=False, extra=None):
    """Every cell of every field against the band model (BAR) and the exact region against the heap
    oracle (EXACT); recorded before anything is asserted."""
    worst, worst_x, same, cells, xcells, xsame, bad = 0.0, 0.0, 0, 0, 0, 0, None
    for s, T in zip(srcs, fields):
        B = FC.model_field(case, s, vmax)[0]
        H = FC.heap_field(case, s)
        assert T.shape == B.shape == FC.fine_shape(case)
        ex = np.ones(B.shape, dtype=bool) if whole else FC.exact_region(case, s, vmax)
        if np.isfinite(T).all():
            m = float(np.max(np.abs(T - B) / np.maximum(B, 1e-300)))
            mx = float(np.max(np.abs(T - H)[ex] / np.maximum(H[ex], 1e-300)))
        else:
            m = mx = float("inf")
        if bad is None or m > worst or mx > worst_x:
            bad = (s, m, mx)
        worst, worst_x = max(worst, m), max(worst_x, mx)
        same += int(np.sum(T == B))
        cells += T.size
        xcells += int(ex.sum())
        xsame += int(np.sum(T[ex] == H[ex]))
    rec = {"rel_max": worst, "exact_rel_max": worst_x, "exact_frac": same / cells, "fields": len(srcs), "cells": cells,
           "exact_cells": xcells, "exact_cells_bit_equal": xsame, "vmax_rel_to_cpu": abs(vmax - FC.model_vmax(case)) / vmax}
    rec.update(extra or {})
    envelope["finer_small/" + group] = rec
    assert worst <= BAR and worst_x <= EXACT, (group, bad, rec)
    assert xsame == xcells, (group, rec)  # the exact region: the heap oracle's bits (module docstring)


@contextlib.contextmanager
def _options(c, **kw):
    old = {k: c.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            c.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            c.set_option(k, v)


@pytest.mark.parametrize("case", FC.MODEL_CASES + FC.SHAPE_CASES, ids=lambda c: c.name)
def test_models_and_shapes(ctx, envelope, case):
    """Every model at subgrid 3, 5 and 9 on the default grid, and the shapes from 2 x 2 up on iso
    and mixed: all sources of the case in one call, every field held to both bars, the whole-field
    cases (4 x 5) to EXACT in every cell; the LDS walk hands no source on (the CPU heap peaks at
    1124 entries at most)."""
    vmax = _set_model(ctx, case)
    srcs = FC.case_sources(case)
    F = _travel(ctx, case, srcs)
    redo = ctx.get_option("exact_redo")
    _vs_refs(envelope, "model/" + case.name, case, srcs, F, vmax, whole=case in FC.WHOLE_CASES,
             extra={"members": int(ctx.get_option("last_k")), "exact_redo": redo})
    assert redo == 0


@pytest.mark.parametrize("case", FC.PARAM_CASES + [FC.FAR_CASE, FC.FAR5_CASE], ids=lambda c: c.name)
def test_parameters(ctx, envelope, case):
    """Each option and host parameter alone, on a fresh context: exact_r 0, 4 and 48 at subgrid 3
    and 9, cdelta 0.1, r0 0 and 10, dnx 2e-4, dnz != dnx, the far band at subgrid 3 (far_sg 3:
    engaged, the field differs from the one-width field) and at subgrid 5 (off: the bits of a
    context without the far options)."""
    srcs = FC.case_sources(case)
    with _context(ctx, case) as c:
        vmax = _set_model(c, case)
        F = _travel(c, case, srcs)
        _vs_refs(envelope, "param/" + case.name, case, srcs, F, vmax)
    if case is FC.FAR_CASE:
        for s, T in zip(srcs, F):
            assert int(np.sum(T != FC.model_field(FC.FAR_OFF_CASE, s, vmax)[0])) > T.size // 10, s
    if case is FC.FAR5_CASE:
        assert _set_model(ctx, FC.FAR5_OFF_CASE) == vmax
        assert np.array_equal(F, _travel(ctx, FC.FAR5_OFF_CASE, srcs))


def test_origin_changes_no_bit(ctx, envelope):
    """A grid origin (sources given in the shifted coordinates) gives the bits of the zero-origin run."""
    srcs = FC.case_sources(FC.ORIGIN_CASE)
    v0 = _set_model(ctx, FC.ORIGIN_ZERO)
    Z = _travel(ctx, FC.ORIGIN_ZERO, srcs)
    vmax = _set_model(ctx, FC.ORIGIN_CASE)
    assert vmax == v0
    F = _travel(ctx, FC.ORIGIN_CASE, srcs)
    _vs_refs(envelope, "param/origin", FC.ORIGIN_CASE, srcs, F, vmax)
    assert np.array_equal(F, Z)


@pytest.mark.parametrize("case", [c for c in FC.MODEL_CASES if c.sg in (3, 9)], ids=lambda c: c.name)
def test_both_walks_give_the_same_bits(ctx, envelope, case):
    """Every models case at subgrid 3 and 9 again with exact_lds 0 (the HBM walk, fmm_exact.hip):
    the bits of the LDS walk (fmm_exact_lds.hip), which test_models_and_shapes holds to both bars."""
    _set_model(ctx, case)
    srcs = FC.case_sources(case)
    L = _travel(ctx, case, srcs)
    with _options(ctx, exact_lds=0):
        assert ctx.get_option("exact_lds") == 0
        Hb = _travel(ctx, case, srcs)
        assert ctx.get_option("exact_redo") == 0
    assert ctx.get_option("exact_lds") == 1
    same = [bool(np.array_equal(L[i], Hb[i])) for i in range(len(srcs))]
    envelope["finer_small/walks/" + case.name] = {"fields": len(srcs), "bit_equal": int(sum(same))}
    assert all(same), (case.name, [srcs[i] for i in range(len(srcs)) if not same[i]])


@pytest.mark.parametrize("case", FC.HBM_CASES + FC.WHOLE_HBM_CASES + [FC.HBM13_CASE], ids=lambda c: c.name)
def test_hbm_walk_past_the_lds_capacity(ctx, envelope, case):
    """Subgrid 11 (12 x 9 on grain and many_mid, 4 x 5 with the whole field inside the prefix) and
    one source at subgrid 13: the LDS walk does not fit (its stage-1 grid is 487^2), fmm_exact.hip
    is the only walk; both bars."""
    vmax = _set_model(ctx, case)
    srcs = FC.case_sources(case)
    F = _travel(ctx, case, srcs)
    _vs_refs(envelope, "hbm/" + case.name, case, srcs, F, vmax, whole=case in FC.WHOLE_CASES,
             extra={"exact_redo": ctx.get_option("exact_redo")})
    assert ctx.get_option("exact_redo") == 0


@contextlib.contextmanager
def _geometry(c, stripe_log, members):
    try:
        c.set_option("stripe_log", stripe_log)
        c.set_option("members", members)
        yield
    finally:
        c.set_option("members", 0)
        c.set_option("stripe_log", 0)


@pytest.mark.parametrize("case", FC.MEMBER_CASES, ids=lambda c: c.name)
def test_every_member_count_gives_one_members_bits(ctx, envelope, case):
    """Subgrid 3 and 5 on mixed and many_mid, 8-column stripes (the last one a single column), 1 to 16
    members: the bits of the one-member run, which meets both bars; the member count in force is
    the one asked for, clamped to the stripe count (13 stripes at subgrid 3); once more with the
    write-through exchange (xcd_local 0)."""
    vmax = _set_model(ctx, case)
    srcs = [FC.case_sources(case)[k] for k in FC.MEMBER_SOURCES]
    nstripes = (FC.fine_shape(case)[1] + 7) // 8
    with _geometry(ctx, 3, 1):
        ref = _travel(ctx, case, srcs)
        assert ctx.get_option("last_k") == 1
    _vs_refs(envelope, "members/" + case.name, case, srcs, ref, vmax)
    ran = []
    for K in range(2, 17):
        with _geometry(ctx, 3, K):
            F = _travel(ctx, case, srcs)
            ran.append(int(ctx.get_option("last_k")))
        assert ran[-1] == min(K, nstripes), (K, ran[-1], nstripes)
        assert np.array_equal(F, ref), (case.name, K)
    with _options(ctx, xcd_local=0), _geometry(ctx, 3, 5):
        F = _travel(ctx, case, srcs)
        assert ctx.get_option("last_k") == 5
    assert np.array_equal(F, ref), case.name
    envelope["finer_small/members/" + case.name]["members_ran"] = ran


def test_batches_positions_and_a_reused_arena(ctx, envelope):
    """A batch equals single-source calls bit for bit; a source's field does not depend on its
    position in the call; after calls at subgrid 9, 3, 1 and 3 again on one context the last equals
    a fresh context's bits (stale S / Tb of the larger earlier call)."""
    import _alifmm

    c3, c9 = FC.MODEL_CASES[FC.MODELS.index("mixed") * 3], FC.MODEL_CASES[FC.MODELS.index("mixed") * 3 + 2]
    assert (c3.name, c9.name) == ("mixed_sg3", "mixed_sg9")
    srcs = FC.case_sources(c3)
    vmax = _set_model(ctx, c3)
    B = _travel(ctx, c3, srcs)
    _vs_refs(envelope, "batch/" + c3.name, c3, srcs, B, vmax)
    for i, s in enumerate(srcs):
        assert np.array_equal(_travel(ctx, c3, [s])[0], B[i]), s
    R = _travel(ctx, c3, srcs[::-1])
    assert np.array_equal(R[::-1], B)
    trio = _travel(ctx, c3, [srcs[3], srcs[8], srcs[3]])
    assert np.array_equal(trio[0], B[3]) and np.array_equal(trio[1], B[8]) and np.array_equal(trio[2], B[3])
    # the arena: larger call first
    c = _alifmm.Context(0)
    try:
        _set_model(c, c9)
        F9 = _travel(c, c9, srcs)
        F3a = _travel(c, c3, srcs)
        xy = [FC.source_xy(c3, s) for s in srcs]
        c.travel([p[0] for p in xy], [p[1] for p in xy], subgrid=1)
        F3b = _travel(c, c3, srcs)
    finally:
        c.close()
    _vs_refs(envelope, "arena/" + c9.name, c9, srcs, F9, vmax)
    assert np.array_equal(F3a, B) and np.array_equal(F3b, B)


@pytest.mark.parametrize("case", FC.SG1_CASES, ids=lambda c: c.name)
def test_subgrid1_prefix_over_the_whole_grid(ctx, envelope, case):
    """6 x 7 and 9 x 12 at subgrid 1: the whole grid lies inside the exact prefix of the source init
    (exact_r 20), the band kernel starts from an empty close list, and every cell equals the heap
    oracle (oracle.travel, correctly rounded build) within EXACT."""
    veln, velpn, vm, sd = FC.model_arrays(case.model, case.nz, case.nx)
    ctx.set_model(veln, velpn, vm, sd, FC.TABLE, FC.TABLE, case.dnx, case.dnz, case.gox, case.goz)
    srcs = FC.case_sources(case)
    F = _travel(ctx, case, srcs)
    worst, same, cells = 0.0, 0, 0
    for s, T in zip(srcs, F):
        H = FC.heap_field(case, s)
        m = float(np.max(np.abs(T - H) / np.maximum(H, 1e-300))) if np.isfinite(T).all() else float("inf")
        worst = max(worst, m)
        same += int(np.sum(T == H))
        cells += T.size
    envelope["finer_small/sg1_whole/" + case.name] = {"exact_rel_max": worst, "exact_frac": same / cells,
                                                      "fields": len(srcs), "cells": cells}
    assert worst <= EXACT, (case.name, worst)


def test_drop_in_surface(ctx):
    """Anis_TTF_rays.travel_finer_grid returns the bits and the shape of ctx.travel(subgrid=sg); an
    even subgrid and a source off the grid raise the library's argument errors."""
    import _alifmm
    import Anis_TTF_rays as A

    case = FC.MODEL_CASES[FC.MODELS.index("grain") * 3 + 1]
    assert case.name == "grain_sg5"
    veln, velpn, vm, sd = FC.model_arrays(case.model, case.nz, case.nx)
    s = FC.case_sources(case)[7]
    x, z = FC.source_xy(case, s)
    _set_model(ctx, case)
    ref = _travel(ctx, case, [s])[0]
    T = A.travel_finer_grid(x, z, veln, velpn, vm, sd, case.sg, FC.TABLE, FC.TABLE, case.gox, case.goz, case.dnx,
                            case.dnz)
    assert T.shape == FC.fine_shape(case) and T.dtype == np.float64 and np.array_equal(T, ref)
    with pytest.raises(_alifmm.AlifmmError, match="even subgrid|subgrid must be odd"):
        ctx.travel([x], [z], subgrid=4)
    with pytest.raises(_alifmm.AlifmmError, match="outside the grid"):
        ctx.travel([case.dnx * (case.nx + 2)], [z], subgrid=case.sg)
    assert np.array_equal(_travel(ctx, case, [s])[0], ref)  # the context still works after both
