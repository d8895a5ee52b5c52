"""alifmm_travel_seeded (include/alifmm.h, csrc/fmm_seed.hip + the band kernel) against its CPU
statement tests/seed_ref.py on the matrix of tests/seed_cases.py, and the contract's other terms:
member counts, batching, the two time sources, copy-out, untouched slots, init_reuse, the errors,
and the drop-in layer (ALI_FMM.skip_fields, ALI_FMM.tfm(tx_path="skip")).  Run on the GPU box:
pytest -m gpu.

The bar is the project's for the device against the CPU band model (tests/test_gpu_band_small.py):
max |T - B| / max(B, 1e-300) <= 1e-9 over ALL cells; tests/test_seed_ref.py holds the reference
finite and positive off the zero-time seeds, where both are 0.  The band options are read back from
the context.  Every figure goes to the session's envelope under "seeded/..." before it is asserted.

Measured on the MI355X when the file was written: rel_max <= 7.4e-16 over the 44 fields of the
matrix (37 of them bit-equal in every cell, the others in 92.5 % to 99.9 % of the cells), 0 for the
checkerboard, the far band, the member counts and the batch; the half-skip image at 0.0101 of its
bound.
"""
import numpy as np
import pytest

import band_cases as BC
import seed_cases as SC

pytestmark = pytest.mark.gpu

BAR = 1e-9
BAND_OPTS = ("cdelta", "cdelta_far", "r_far", "r0")
E_ARG, E_CAPACITY = "rc=-2", "rc=-3"


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    yield c
    c.close()


def _set_model(c, case):
    veln, velpn, vm, sd = BC.model_arrays(case.model, case.nz, case.nx)
    c.set_model(veln, velpn, vm, sd, BC.TABLE, BC.TABLE, case.dnx, case.dnz, case.gox, case.goz)
    return {k: c.get_option(k) for k in BAND_OPTS}, c.get_option("vmax")


def _incident(c, case, srcs, first_slot=0):
    xy = [BC.source_xy(case, s) for s in srcs]
    c.travel([p[0] for p in xy], [p[1] for p in xy], first_slot=first_slot, copy_out=False)


def _vs_ref(envelope, name, case, s, t, T, opt, vmax):
    B = SC.ref_field(case, s, t, opt, vmax)
    assert T.shape == B.shape
    rel = np.abs(T - B) / np.maximum(B, 1e-300)
    m = float(np.max(rel)) if np.isfinite(T).all() else float("inf")
    envelope["seeded/" + name] = {"rel_max": m, "exact_frac": float(np.mean(T == B)), "seeds": len(s.iz)}
    print("seeded/%s: rel max %.3e, exact %.4f" % (name, m, float(np.mean(T == B))))
    assert m <= BAR, (name, m, np.unravel_index(int(np.argmax(rel)), rel.shape))
    assert np.array_equal(T[s.iz, s.ix], t), name  # the seeds keep their times bit for bit


@pytest.mark.parametrize("model,nz,nx", SC.MODEL_GRIDS)
def test_matrix_equals_seed_ref(ctx, envelope, model, nz, nx):
    """Every seed set on every model: rows on the top, the bottom (times gathered from a resident
    point-source field) and the interior (steered host times), two layers, single nodes on and next
    to the stripe boundary at column 64, vertical lines there, a staircase, scattered nodes."""
    case = SC.case(model, nz, nx)
    opt, vmax = _set_model(ctx, case)
    _incident(ctx, case, [SC.INCIDENT(nz, nx)])
    inc = ctx.get_field(0, 1)
    failed = []
    for s in SC.seed_sets(nz, nx, vmax):
        if s.t is None:
            t = SC.incident_times(case, s, inc)
            T = ctx.travel_seeded(s.iz, s.ix, from_slots=[0], first_slot=1)[0]
        else:
            t = s.t
            T = ctx.travel_seeded(s.iz, s.ix, times=t, first_slot=1)[0]
        assert ctx.get_option("seed_nodes") == len(s.iz)
        try:
            _vs_ref(envelope, "matrix/%s/%s" % (case.name, s.name), case, s, t, T, opt, vmax)
        except AssertionError as e:  # every set's figure is recorded before the case fails
            failed.append(str(e)[:300])
    assert not failed, failed


def test_checkerboard_hands_over_every_cell(ctx, envelope):
    """97 x 122, every second node a seed: 5 917 + 5 917 = 11 834 entries, a close list past the band
    kernel's LDS capacity from the first step."""
    case = SC.case(*SC.CHECKER_FITS)
    opt, vmax = _set_model(ctx, case)
    s = SC.checkerboard(case.nz, case.nx, vmax)
    T = ctx.travel_seeded(s.iz, s.ix, times=s.t)[0]
    assert (ctx.get_option("seed_nodes"), ctx.get_option("seed_close")) == (5917, 5917)
    _vs_ref(envelope, "checkerboard", case, s, s.t, T, opt, vmax)


def test_far_band(envelope):
    """A fresh context with the far band moved in (r_far 20 cells): engaged, and as the reference's."""
    import _alifmm

    case = BC.case("seed_far", SC.FAR_GRID[0], SC.FAR_GRID[1:], opts=SC.FAR_OPTS, dnx=SC.DNX)
    off = BC.case("seed_far_off", SC.FAR_GRID[0], SC.FAR_GRID[1:], opts={"cdelta_far": 0.0}, dnx=SC.DNX)
    c = _alifmm.Context(0)
    try:
        for k, v in case.opts.items():
            c.set_option(k, v)
        opt, vmax = _set_model(c, case)
        assert opt["r_far"] == 20 and opt["cdelta_far"] == 0.7
        s = SC.seed_sets(case.nz, case.nx, vmax)[0]
        T = c.travel_seeded(s.iz, s.ix, times=s.t)[0]
        _vs_ref(envelope, "far", case, s, s.t, T, opt, vmax)
        G = SC.ref_field(off, s, s.t, dict(opt, cdelta_far=0.0), vmax)
        assert int(np.sum(T != G)) > 1000
    finally:
        c.close()


THIRTEEN = lambda case: BC.sources(case.nz, case.nx)  # noqa: E731


def _reflect13(c, case, s, **kw):
    """13 incident fields in slots 0 .. 12, their reflected fields off seed set s in 13 .. 25."""
    _incident(c, case, THIRTEEN(case))
    c.travel_seeded(s.iz, s.ix, from_slots=list(range(13)), first_slot=13, copy_out=False, **kw)
    return c.copy_fields(13, 13, 1)[0]


def test_every_member_count_gives_one_members_bits(ctx, envelope):
    """stripe_log 3 with 1 .. 16 members and the automatic choice: the one-member bits, which are the
    reference's."""
    case = SC.case("mixed", 41, 127)
    opt, vmax = _set_model(ctx, case)
    s = SC.seed_sets(case.nz, case.nx, vmax)[1]
    assert s.name == "bottom_from"
    try:
        ctx.set_option("stripe_log", 3)
        ctx.set_option("members", 1)
        ref = _reflect13(ctx, case, s)
        assert ctx.get_option("last_k") == 1
        for i in (0, 5, 12):
            _vs_ref(envelope, "members/field%d" % i, case, s, SC.incident_times(case, s, ctx.get_field(i, 1)), ref[i],
                    opt, vmax)
        ran = []
        for K in list(range(2, 17)) + [0]:
            ctx.set_option("members", K)
            ctx.set_option("stripe_log", 3 if K else 0)
            F = _reflect13(ctx, case, s)
            k = int(ctx.get_option("last_k"))
            ran.append(k)
            assert k == K or (K == 0 and k >= 1), (K, k)
            assert np.array_equal(F, ref), (K, [i for i in range(13) if not np.array_equal(F[i], ref[i])])
        envelope["seeded/members/ran"] = ran
        # the write-through exchange (the path members on different XCDs take): the same bits
        ctx.set_option("xcd_local", 0)
        ctx.set_option("members", 4)
        ctx.set_option("stripe_log", 3)
        assert np.array_equal(_reflect13(ctx, case, s), ref) and ctx.get_option("last_k") == 4
    finally:
        ctx.set_option("xcd_local", 1)
        ctx.set_option("members", 0)
        ctx.set_option("stripe_log", 0)


def test_batches_time_sources_and_copy_out(ctx, envelope):
    """13 fields with different from_slots in one call equal each alone and the same call in chunks
    of 5 (option batch); from_slots equals times = the source field at the nodes; out equals the
    resident slots; the source slots and a bystander slot keep their bits."""
    case = SC.case("grain", 61, 65)
    opt, vmax = _set_model(ctx, case)
    s = SC.seed_sets(case.nz, case.nx, vmax)[1]
    _incident(ctx, case, THIRTEEN(case))
    inc = ctx.copy_fields(0, 13, 1)[0]
    bystander = np.full((case.nz, case.nx), 7.25)
    ctx.put_field(30, 1, bystander)
    out = ctx.travel_seeded(s.iz, s.ix, from_slots=list(range(13)), first_slot=13)
    assert ctx.get_option("seed_close") == case.nx and ctx.get_option("seed_ms") > 0
    init_ms, band_ms, total_ms = ctx.last_timing()
    assert init_ms > 0 and band_ms > 0 and total_ms >= band_ms
    assert ctx.source_stats(13)[0][3] > 0
    res = ctx.copy_fields(13, 13, 1)[0]
    assert np.array_equal(out, res)
    assert np.array_equal(ctx.copy_fields(0, 13, 1)[0], inc)
    assert np.array_equal(ctx.get_field(30, 1), bystander)
    _vs_ref(envelope, "batch/field3", case, s, SC.incident_times(case, s, inc[3]), out[3], opt, vmax)
    for i in range(13):
        one = ctx.travel_seeded(s.iz, s.ix, from_slots=[i], first_slot=13)
        assert np.array_equal(one[0], out[i]), i
    try:
        ctx.set_option("batch", 5)
        assert np.array_equal(ctx.travel_seeded(s.iz, s.ix, from_slots=list(range(13)), first_slot=13), out)
    finally:
        ctx.set_option("batch", 256)
    host = ctx.travel_seeded(s.iz, s.ix, times=inc[:, s.iz, s.ix], first_slot=13)
    assert np.array_equal(host, out)
    assert np.array_equal(ctx.copy_fields(0, 13, 1)[0], inc)


def test_every_node_a_seed_returns_the_seeds(ctx):
    """No close cell at all (61 x 65 = 3 965 seeds): the band has nothing to do and the field is the
    seed times, bit for bit, for one member and for several."""
    case = SC.case("grain", 61, 65)
    _, vmax = _set_model(ctx, case)
    zz, xx = np.mgrid[0:case.nz, 0:case.nx]
    iz, ix = zz.ravel().astype(np.int32), xx.ravel().astype(np.int32)
    t = np.hypot(iz * case.dnz, ix * case.dnx) / vmax
    try:
        for K in (1, 4, 0):
            ctx.set_option("stripe_log", 3 if K else 0)
            ctx.set_option("members", K)
            T = ctx.travel_seeded(iz, ix, times=t)[0]
            assert (ctx.get_option("seed_nodes"), ctx.get_option("seed_close")) == (case.nz * case.nx, 0)
            assert np.array_equal(T.ravel(), t), K
    finally:
        ctx.set_option("members", 0)
        ctx.set_option("stripe_log", 0)


@pytest.mark.parametrize("nfield", [3, 20])
def test_init_reuse_is_untouched(nfield):
    """travel of 13 sources, travel_seeded of fewer (3) and of more (20) fields into other slots, the
    same travel again: every walk is skipped and the fields have the first call's bits; the init
    profile reports the same walks right after the seeded call.  A fresh context: the work arena
    starts from the travel call's size."""
    import _alifmm

    case = SC.case("mixed", 41, 127)
    c = _alifmm.Context(0)
    try:
        _set_model(c, case)
        s = SC.seed_sets(case.nz, case.nx, c.get_option("vmax"))[1]
        xy = [BC.source_xy(case, p) for p in THIRTEEN(case)]
        x, z = [p[0] for p in xy], [p[1] for p in xy]
        F1 = c.travel(x, z)
        prof = c.init_profile(3)
        R = c.travel_seeded(s.iz, s.ix, from_slots=[(5 * i + 2) % 13 for i in range(nfield)], first_slot=13)
        assert np.isfinite(R).all()
        assert np.array_equal(c.init_profile(3), prof)
        F2 = c.travel(x, z)
        assert c.get_option("init_reused") == 13
        assert np.array_equal(F1, F2)
    finally:
        c.close()


def test_travel_of_another_size_in_between_keeps_the_hand_overs():
    """The same for plain travel calls: 13 sources, the first 3 of them again into other slots (another
    member count: the rest of the work arena is regrown), then the 13 again: every walk after the
    first call's is skipped, and the fields have the first call's bits."""
    import _alifmm

    case = SC.case("mixed", 41, 127)
    c = _alifmm.Context(0)
    try:
        _set_model(c, case)
        xy = [BC.source_xy(case, p) for p in THIRTEEN(case)]
        x, z = [p[0] for p in xy], [p[1] for p in xy]
        F1 = c.travel(x, z)
        F3 = c.travel(x[:3], z[:3], first_slot=13)
        assert c.get_option("init_reused") == 3
        assert np.array_equal(F3, F1[:3])
        F2 = c.travel(x, z)
        assert c.get_option("init_reused") == 13
        assert np.array_equal(F1, F2)
    finally:
        c.close()


def test_errors_leave_the_context_usable(ctx):
    import _alifmm

    case = SC.case("grain", 61, 65)
    _set_model(ctx, case)
    ctx.release_fields()
    nz, nx = case.nz, case.nx
    src = BC.source_xy(case, (20, 3))
    base = ctx.travel([src[0]], [src[1]])[0]
    row = np.full(nx, nz - 1, dtype=np.int32), np.arange(nx, dtype=np.int32)
    zero = np.zeros(nx)

    def refused(code, *a, **kw):
        with pytest.raises(_alifmm.AlifmmError) as e:
            ctx.travel_seeded(*a, **kw)
        assert code in str(e.value), str(e.value)
        assert np.array_equal(ctx.travel([src[0]], [src[1]])[0], base)

    def bad_time(v):
        t = zero.copy()
        t[17] = v
        return t

    refused(E_ARG, [], [], times=np.zeros((1, 0)), first_slot=1)                    # nseed < 1
    refused(E_ARG, row[0], row[1], times=np.zeros((0, nx)), first_slot=1)           # nfield < 1
    refused(E_ARG, [nz], [0], times=[0.0], first_slot=1)                            # outside the grid
    refused(E_ARG, [0], [-1], times=[0.0], first_slot=1)
    refused(E_ARG, [3, 4, 3], [5, 5, 5], times=[0.0, 0.0, 0.0], first_slot=1)       # listed twice
    refused(E_ARG, row[0], row[1], times=zero, from_slots=[0], first_slot=1)        # both
    refused(E_ARG, row[0], row[1], first_slot=1)                                    # neither
    refused(E_ARG, row[0], row[1], from_slots=[99], first_slot=1)                   # empty slot
    refused(E_ARG, row[0], row[1], from_slots=[1], first_slot=1)                    # inside the destination
    refused(E_ARG, row[0], row[1], from_slots=[0, 2], first_slot=1)
    for v in (np.nan, np.inf, -1e-9, -0.0):
        refused(E_ARG, row[0], row[1], times=bad_time(v), first_slot=1)
    for v in (np.nan, np.inf, -1e-9):                                               # gathered times
        f = base.copy()
        f[nz - 1, 17] = v
        ctx.put_field(5, 1, f)
        refused(E_ARG, row[0], row[1], from_slots=[5], first_slot=1)
    ctx.travel([src[0]], [src[1]], subgrid=3, first_slot=6, copy_out=False)        # not subgrid 1
    refused(E_ARG, row[0], row[1], from_slots=[6], first_slot=1)
    # a field of another shape, left from another model
    small = SC.case("grain", 41, 65)
    _set_model(ctx, small)
    ctx.travel([src[0]], [src[1]], first_slot=7, copy_out=False)
    _set_model(ctx, case)
    refused(E_ARG, row[0], row[1], from_slots=[7], first_slot=1)
    good = ctx.travel_seeded(row[0], row[1], from_slots=[0], first_slot=1)
    assert np.isfinite(good).all()


def test_no_model_is_refused():
    import _alifmm

    c = _alifmm.Context(0)
    try:
        with pytest.raises(_alifmm.AlifmmError) as e:
            c.travel_seeded([0], [0], times=[0.0])
        assert E_ARG in str(e.value)
    finally:
        c.close()


def test_capacity_is_refused_before_any_launch(ctx):
    """The checkerboard on 97 x 129 needs 12 513 entries: ALIFMM_E_CAPACITY, the destination slot
    as it was, a plain travel as before."""
    import _alifmm

    case = SC.case(*SC.CHECKER_OVER)
    _, vmax = _set_model(ctx, case)
    ctx.release_fields()
    src = BC.source_xy(case, (40, 0))
    base = ctx.travel([src[0]], [src[1]])[0]
    s = SC.checkerboard(case.nz, case.nx, vmax)
    with pytest.raises(_alifmm.AlifmmError) as e:
        ctx.travel_seeded(s.iz, s.ix, times=s.t, first_slot=0)
    assert E_CAPACITY in str(e.value) and "exceed" in str(e.value), str(e.value)
    assert ctx.get_option("seed_nodes") + ctx.get_option("seed_close") == 12513
    assert np.array_equal(ctx.get_field(0, 1), base)
    assert np.array_equal(ctx.travel([src[0]], [src[1]])[0], base)


def test_drop_in_half_skip_tfm_and_skip_fields(envelope):
    """ALI_FMM.tfm(tx_path="skip") equals tests/tfm_ref.py fed the fields read back from the slots (the
    comparison of test_gpu_tfm.py::test_slot_lists); ALI_FMM.skip_fields equals
    Context.travel_seeded on the same inputs."""
    import _alifmm
    import Anis_TTF_rays as A
    import tfm_ref as R
    import workloads as W

    nz, nx = R.NZ, R.NX
    veln, velpn, vm = np.zeros((nz, nx)), np.ones((nz, nx), dtype=np.int64), np.full((nz, nx), R.SPEED)
    tab = W.default_table()
    ex = R.element_x(9)
    scx, scz = [float(x) * R.DNX for x in ex], [0.0] * 9
    a = A.ALI_FMM(veln, velpn, vm, scx, scz, group_vel=tab, phase_vel=tab, stif_den=None, dnx=R.DNX)
    wall = np.full(nx, nz - 1, dtype=np.int32), np.arange(nx, dtype=np.int32)
    tx, rx = [8, 4, 4, 1, 0], list(range(9))
    fmc = R.data(5, 9, seed=6)
    img = a.tfm(fmc, R.FS, t0=R.T0, tx=tx, rx=rx, tx_path="skip", reflector=wall)
    c = a._ctx(0)
    slots = a.skip_slots
    assert not set(slots["direct"].values()) & set(slots["skip"].values())
    Tt = np.stack([c.get_field(slots["skip"][i], 1) for i in tx])
    Tr = np.stack([c.get_field(slots["direct"][i], 1) for i in rx])
    assert np.isfinite(Tt).all() and (Tt[:, :-1] > Tr[tx][:, :-1]).all()  # off the wall the reflected leg is later
    ref, mag, cnt = R.tfm_ref(Tt, Tr, fmc, R.FS, R.T0)
    r = R.worst_ratio(img, ref, 45, mag)
    envelope["seeded/tfm_half_skip"] = r
    print("seeded/tfm_half_skip: worst |I - I_ref| / bound = %.3g" % r)
    assert img.shape == ref.shape and r <= 1.0, r
    with pytest.raises(ValueError):
        a.tfm(fmc, R.FS, t0=R.T0, tx=tx, rx=rx, tx_path="skip")
    S = a.skip_fields(wall[0], wall[1], copy_out=True)
    own = _alifmm.Context(0)
    try:
        own.set_model(veln, velpn, vm, None, tab, tab, R.DNX)
        own.travel(scx, scz, copy_out=False)
        T = own.travel_seeded(wall[0], wall[1], from_slots=list(range(9)), first_slot=9)
    finally:
        own.close()
    assert np.array_equal(S, T)
