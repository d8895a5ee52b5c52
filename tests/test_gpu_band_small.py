"""The band kernel (csrc/fmm_band_k.hip) against the CPU band model (oracle/band_model.c: the same
band-synchronous algorithm, local operators and schedule) on the small-shape matrix of
tests/band_cases.py: every material path, non-square and ragged grids, sources on corners, edges
and stripe boundaries, every member count, batches, origin and spacing, the streamed copy-out and
the write-through exchange.  Run on the GPU box: pytest -m gpu.

The bar is the project's for this comparison (tests/test_gpu_parity.py): max |T - B| / B <= 1e-9 over
ALL cells (tests/test_oracle.py::test_band_case_matrix_preconditions: the model is finite and
positive everywhere but at the source, where both are 0).  The measured values and the bit-exact
fractions go to the session's parity envelope (conftest.py `envelope`) under "band_small/...".
The heap oracle is not consulted here: the 401^2 tests of test_gpu_parity.py own that bar.

Measured on the MI355X when the file was written: rel_max <= 2.2e-15 in every group, 97.3 % to
100 % of the cells bit-equal (the rest: glibc's trigonometric functions against the device's
correctly rounded ones); the bar stays where the project has it.  The matrix found two device
bugs, both in the source initialisation and both fixed with it: exact_r below 7 wrote the stage-3
hand-over outside the prefix window (fmm_init.hip), and the lane-parallel stencil selection took
nodes past update()'s quirk bound for interior ones (local_ops.h update_select_lanes; the mixed
model, source on the left edge at mid height, 2.9e-4).
"""
import contextlib

import numpy as np
import pytest

import band_cases as BC

pytestmark = pytest.mark.gpu

BAR = 1e-9
BAND_OPTS = ("cdelta", "cdelta_far", "r_far", "r0", "exact_r")


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
    veln, velpn, vm, sd = BC.model_arrays(case.model, case.nz, case.nx)
    c.set_model(veln, velpn, vm, sd, BC.TABLE, BC.TABLE, case.dnx, case.dnz, case.gox, case.goz)
    opt = {k: c.get_option(k) for k in BAND_OPTS}
    want = BC.lib_options(case)  # what the CPU precondition test ran the model with
    for k in BAND_OPTS:
        assert abs(opt[k] - want[k]) <= 1e-15, (case.name, k, opt[k], want[k])
    return opt, c.get_option("vmax")


def _travel(c, case, srcs):
    """Fields of the sources of one call, left resident, read back slot by slot."""
    xy = [BC.source_xy(case, s) for s in srcs]
    c.travel([p[0] for p in xy], [p[1] for p in xy], copy_out=False)
    return [c.get_field(i, 1) for i in range(len(srcs))]


def _travel_stack(c, case, srcs):
    """The same as one (n, nz, nx) array (alifmm_copy_fields of the resident slots)."""
    xy = [BC.source_xy(case, s) for s in srcs]
    c.travel([p[0] for p in xy], [p[1] for p in xy], copy_out=False)
    return c.copy_fields(0, len(srcs), 1)[0]


def _vs_model(envelope, group, case, srcs, fields, opt, vmax, extra=None):
    """Every cell of every field against the band model run with the context's own options; the
    figures are recorded before anything is asserted."""
    worst, exact, cells, bad = 0.0, 0, 0, None
    for s, T in zip(srcs, fields):
        B = BC.model_field(case, s, opt, vmax)
        assert T.shape == B.shape
        rel = np.abs(T - B) / np.maximum(B, 1e-300)
        m = float(np.max(rel)) if np.isfinite(T).all() else float("inf")
        if m > worst or bad is None:
            worst, bad = max(worst, m), (s, m)
        exact += int(np.sum(T == B))
        cells += T.size
    rec = {"rel_max": worst, "exact_frac": exact / cells, "fields": len(srcs), "cells": cells,
           "vmax_rel_to_cpu": abs(vmax - BC.model_vmax(case)) / vmax}
    rec.update(extra or {})
    envelope["band_small/" + group] = rec
    assert worst <= BAR, (group, bad, rec)


@contextlib.contextmanager
def _geometry(c, stripe_log, members):
    try:
        c.set_option("stripe_log", stripe_log)
        c.set_option("members", members)
        yield
    finally:
        c.set_option("members", 0)
        c.set_option("stripe_log", 0)


NMAT = {"iso": lambda n: n == 1, "grain": lambda n: 1 < n <= 256, "mixed": lambda n: 100 < n <= 256,
        "many_mid": lambda n: 256 < n <= 4096, "many_big": lambda n: n == 0}


@pytest.mark.parametrize("case", BC.MODEL_CASES, ids=lambda c: c.name)
def test_models_equal_band_model(ctx, envelope, case):
    """Every material path at the default geometry, all 13 sources in one call (the batch pads to
    16): one record; few records; the LDS table with byte ids and table / Christoffel materials
    side by side; ids and records in HBM; no ids at all."""
    opt, vmax = _set_model(ctx, case)
    assert NMAT[case.model](int(ctx.get_option("nmat"))), (case.name, ctx.get_option("nmat"))
    srcs = BC.sources(case.nz, case.nx)
    assert len(srcs) == 13 and len(set(srcs)) == 13
    F = _travel(ctx, case, srcs)
    _vs_model(envelope, "model/" + case.name, case, srcs, F, opt, vmax, {"members": int(ctx.get_option("last_k"))})


@pytest.mark.parametrize("case", BC.SHAPE_CASES, ids=lambda c: c.name)
def test_shapes_equal_band_model(ctx, envelope, case):
    """Non-square grids, a last stripe of one column (129) and of W - 1 (127), two rows, three
    columns; sources on the corners, the edges and the stripe-boundary columns."""
    opt, vmax = _set_model(ctx, case)
    srcs = BC.sources(case.nz, case.nx)
    F = _travel(ctx, case, srcs)
    _vs_model(envelope, "shape/" + case.name, case, srcs, F, opt, vmax, {"members": int(ctx.get_option("last_k"))})


@pytest.mark.parametrize("case", BC.PARAM_CASES + [BC.FAR_CASE], ids=lambda c: c.name)
def test_parameters_equal_band_model(ctx, envelope, case):
    """Each option and host parameter alone: cdelta 0.1, exact_r 4 and 48, r0 0 and 10, the far band
    (engaged: the field differs from the model's one-width field), dnx 2e-4, dnz != dnx."""
    with _context(ctx, case) as c:
        opt, vmax = _set_model(c, case)
        for k, v in case.opts.items():
            assert c.get_option(k) == v, (case.name, k)
        all_srcs = BC.sources(case.nz, case.nx)
        srcs = [BC.FAR_SOURCE] if case is BC.FAR_CASE else [all_srcs[k] for k in BC.PARAM_SOURCES]
        F = _travel(c, case, srcs)
        _vs_model(envelope, "param/" + case.name, case, srcs, F, opt, vmax)
        if case is BC.FAR_CASE:
            assert int(np.sum(F[0] != BC.model_field(BC.FAR_OFF_CASE, BC.FAR_SOURCE))) > 10000


def test_origin_changes_no_bit(ctx, envelope):
    """A grid origin (gox, goz = 0.0125, -0.003; sources given in the shifted coordinates) gives the
    bits of the zero-origin run, and the model's run with that origin."""
    srcs = [BC.sources(*BC.DEFAULT_SHAPE)[k] for k in BC.PARAM_SOURCES]
    opt0, vmax0 = _set_model(ctx, BC.ORIGIN_ZERO)
    Z = _travel(ctx, BC.ORIGIN_ZERO, srcs)
    opt, vmax = _set_model(ctx, BC.ORIGIN_CASE)
    assert (opt, vmax) == (opt0, vmax0)
    F = _travel(ctx, BC.ORIGIN_CASE, srcs)
    _vs_model(envelope, "param/origin", BC.ORIGIN_CASE, srcs, F, opt, vmax)
    for s, a, b in zip(srcs, F, Z):
        assert np.array_equal(a, b), s


@pytest.mark.parametrize("case,geoms", [(c, BC.MEMBER_GEOMS) for c in BC.MEMBER_CASES] +
                         [(c, BC.MEMBER_GEOMS_HBM[c.model]) for c in BC.MEMBER_CASES_HBM], ids=lambda v: getattr(v, "name", None))
def test_every_member_count_gives_one_members_bits(ctx, envelope, case, geoms):
    """stripe_log 3 with 1 .. 16 members, stripe_log 4 with 2 and 7, and the automatic choice: every
    run has the member count asked for and the bits of the one-member run, which equals the band
    model (so each of them does).  13 sources per call: corners, edges, stripe-boundary columns."""
    opt, vmax = _set_model(ctx, case)
    srcs = BC.sources(case.nz, case.nx)
    with _geometry(ctx, 3, 1):
        ref = _travel_stack(ctx, case, srcs)
        assert ctx.get_option("last_k") == 1
    _vs_model(envelope, "members/" + case.name, case, srcs, ref, opt, vmax, {"geometries": [list(g) for g in geoms]})
    ran = []
    for slog, K in geoms:
        with _geometry(ctx, slog, K):
            F = _travel_stack(ctx, case, srcs)
            k = int(ctx.get_option("last_k"))
        ran.append(k)
        assert k == K or (K == 0 and k >= 1), (slog, K, k)
        same = [bool(np.array_equal(F[i], ref[i])) for i in range(len(srcs))]
        assert all(same), (case.name, slog, K, [srcs[i] for i in range(len(srcs)) if not same[i]])
    envelope["band_small/members/" + case.name]["members_ran"] = ran
    assert ctx.get_option("members") == 0 and ctx.get_option("stripe_log") == 0


@pytest.mark.parametrize("case,slog,K,kept", BC.NARROW_CASES, ids=lambda v: getattr(v, "name", None))
def test_more_members_than_stripes_is_clamped(ctx, envelope, case, slog, K, kept):
    """16 members asked for on a grid of one (65 x 3) or two (61 x 65) 64-column stripes: the host
    lowers the count to the stripe count (host_travel.cpp choose_members; a member without a stripe would
    still take its 1 / K share of the work-list capacity from the members that own cells), and the
    run gives the one-member bits and the model's field."""
    opt, vmax = _set_model(ctx, case)
    srcs = BC.sources(case.nz, case.nx)
    with _geometry(ctx, slog, 1):
        ref = _travel_stack(ctx, case, srcs)
        assert ctx.get_option("last_k") == 1
    with _geometry(ctx, slog, K):
        F = _travel_stack(ctx, case, srcs)
        assert ctx.get_option("last_k") == kept
    _vs_model(envelope, "narrow/" + case.name, case, srcs, F, opt, vmax, {"asked": K, "ran": kept})
    assert np.array_equal(F, ref)


@pytest.mark.parametrize("slog,K", [(0, 0), (3, 5)])
@pytest.mark.parametrize("case", BC.MODEL_CASES[1:3], ids=lambda c: c.name)
def test_batches_equal_single_runs(ctx, envelope, case, slog, K):
    """13 sources in one call (padded to 16 internally), 3 in one call, and each alone: every slot
    equals the model and the same source run alone, bit for bit; the same source twice in one call
    gives the same field twice."""
    opt, vmax = _set_model(ctx, case)
    srcs = BC.sources(case.nz, case.nx)
    with _geometry(ctx, slog, K):
        B13 = _travel_stack(ctx, case, srcs)
        kb = int(ctx.get_option("last_k"))
        _vs_model(envelope, "batch/%s_s%d_k%d" % (case.name, slog, K), case, srcs, B13, opt, vmax, {"members": kb})
        for i, s in enumerate(srcs):
            one = _travel_stack(ctx, case, [s])
            assert K == 0 or ctx.get_option("last_k") == K
            assert np.array_equal(one[0], B13[i]), (case.name, s)
        trio = [srcs[3], srcs[10], srcs[3]]
        B3 = _travel_stack(ctx, case, trio)
        assert np.array_equal(B3[0], B3[2]) and np.array_equal(B3[0], B13[3]) and np.array_equal(B3[1], B13[10])


@pytest.mark.parametrize("slog,K", BC.STREAM_GEOMS)
@pytest.mark.parametrize("case", BC.STREAM_CASES, ids=lambda c: c.name)
def test_streamed_fields_equal_resident(ctx, envelope, case, slog, K):
    """travel_into on grids whose last tiles are ragged in both directions (97 x 129, 41 x 127), with
    1, 3 and 16 members: the fields streamed tile by tile into non-consecutive rows of a larger
    zeroed stack, in reverse order, equal the resident fields (which equal the model); no other row
    is written."""
    opt, vmax = _set_model(ctx, case)
    srcs = BC.sources(case.nz, case.nx)
    n = len(srcs)
    xy = [BC.source_xy(case, s) for s in srcs]
    with _geometry(ctx, slog, K):
        R = _travel_stack(ctx, case, srcs)
        assert ctx.get_option("last_k") == K
        D = np.zeros((2 * n + 3, case.nz, case.nx))
        rows = [2 * n - 2 * i for i in range(n)]  # 26, 24, ..., 2
        ctx.travel_into([p[0] for p in xy], [p[1] for p in xy], D, rows)
        assert ctx.get_option("last_k") == K
        fb = ctx.get_option("stream_fallback")
    _vs_model(envelope, "stream/%s_k%d" % (case.name, K), case, srcs, R, opt, vmax, {"stream_fallback": fb})
    for i in range(n):
        assert np.array_equal(D[rows[i]], R[i]), (case.name, K, srcs[i])
    for r in range(D.shape[0]):
        assert r in rows or not D[r].any(), r


@pytest.mark.parametrize("K", [2, 16])
@pytest.mark.parametrize("case", BC.MEMBER_CASES, ids=lambda c: c.name)
def test_write_through_exchange_gives_the_same_bits(ctx, envelope, case, K):
    """Option xcd_local 0 keeps the cross-member exchange on write-through (sc1) stores, the path
    members on different XCDs take: the same bits as the default, both equal to the model, and the
    kernel's own count of XCD-local steps (band profile word 12, x 100) is 0 in the forced run.  The
    default run's fraction is recorded, not asserted (placement is read, not assumed)."""
    opt, vmax = _set_model(ctx, case)
    srcs = BC.sources(case.nz, case.nx)
    out = {}
    try:
        ctx.set_option("prof", 1)
        for xl in (1, 0):
            ctx.set_option("xcd_local", xl)
            assert ctx.get_option("xcd_local") == xl
            with _geometry(ctx, 3, K):
                F = _travel_stack(ctx, case, srcs)
                assert ctx.get_option("last_k") == K
            loc = np.array([ctx.band_profile(i)[12] for i in range(len(srcs))], dtype=np.float64)
            steps = np.array([ctx.source_stats(i)[0][3] for i in range(len(srcs))], dtype=np.float64)
            assert (steps > 0).all()
            out[xl] = (F, loc / (100.0 * steps))
    finally:
        ctx.set_option("xcd_local", 1)
        ctx.set_option("prof", 0)
    _vs_model(envelope, "xcd_local/%s_k%d" % (case.name, K), case, srcs, out[0][0], opt, vmax,
              {"local_step_frac_default": float(out[1][1].mean()), "local_step_frac_forced": float(out[0][1].max())})
    assert np.array_equal(out[0][0], out[1][0])
    assert (out[0][1] == 0).all(), out[0][1]
    assert ((out[1][1] >= 0) & (out[1][1] <= 1)).all(), out[1][1]
