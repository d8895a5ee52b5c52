"""The band kernel's long-list paths (fmm_band_k.hip: the lists' spill sides, the counting sort, the
claim passes, the rim read-back, the fallback's rounds and scan) against the CPU models at thin
shapes, and the work-list capacity retry.  The cases and the list census that chose them are in
tests/long_cases.py; tests/test_long_cases_ref.py holds their preconditions on the CPU.  Run on the
GPU box: pytest -m gpu.

Per case: (1) the one-member field against the CPU model (tests/seed_ref.py SeedRef.field_c or
oracle.band_travel, the correctly rounded build) over ALL cells at the project's bar for the device
against the band model, max |T - B| / max(B, 1e-300) <= 1e-9 (tests/test_gpu_band_small.py,
tests/test_gpu_seeded.py); (2) every other member geometry bit-identical to it; (3) with option prof
1, the kernel's own sums (alifmm_band_profile entries 6 .. 9: member 0's close, accepted and evaluated
cells summed over the steps and its largest close set) and its step count equal to the census of the
reference run, exactly: what shows that a run took the long path.  Every figure goes to the session's
envelope under "band_long/..." before it is asserted.

Measured on the MI355X when the file was written: rel_max 0 and exact_frac 1.0 on all 32 one-member
fields (every cell bit-equal to the CPU model), every other member geometry bit-identical, all 65
records and both capacity cases' equal to the census; the file in under 4 s.
"""
import numpy as np
import pytest

import band_cases as BC
import long_cases as LC

pytestmark = pytest.mark.gpu

BAR = 1e-9
BAND_OPTS = ("cdelta", "cdelta_far", "r_far", "r0", "exact_r")


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    yield c
    c.close()


def _set_model(c, case):
    veln, velpn, vm, sd = LC.model_arrays(case)
    c.set_model(veln, velpn, vm, sd, BC.TABLE, BC.TABLE, LC.DNX)
    return {k: c.get_option(k) for k in BAND_OPTS}, c.get_option("vmax")


def _run(c, case, stripe_log, members, prof=0):
    """The case's field in slot 0 under a member geometry; the options are put back."""
    try:
        c.set_option("stripe_log", stripe_log)
        c.set_option("members", members)
        c.set_option("prof", prof)
        if case.kind == "travel":
            c.travel([LC.DNX * case.arg[0]], [LC.DNX * case.arg[1]], copy_out=False)
        else:
            iz, ix, t = LC.seeds_of(case)
            c.travel_seeded(iz, ix, times=t, copy_out=False)
        assert c.get_option("last_k") == members
        return c.get_field(0, 1)
    finally:
        c.set_option("prof", 0)
        c.set_option("members", 0)
        c.set_option("stripe_log", 0)


def _vs_ref(envelope, key, T, B, **more):
    assert T.shape == B.shape
    rel = np.abs(T - B) / np.maximum(B, 1e-300)
    m = float(np.max(rel)) if np.isfinite(T).all() else float("inf")
    envelope["band_long/" + key] = dict({"rel_max": m, "exact_frac": float(np.mean(T == B))}, **more)
    print("band_long/%s: rel max %.3e, exact %.6f %s" % (key, m, float(np.mean(T == B)), more))
    assert m <= BAR, (key, m, np.unravel_index(int(np.argmax(rel)), rel.shape))


def _device_record(c):
    """(member 0's sums of close, accepted and evaluated cells and its largest close set), band steps."""
    return tuple(int(v) for v in c.band_profile(0)[6:10]), int(c.source_stats(0)[0][3])


def _check_case(c, envelope, case):
    opt, vmax = _set_model(c, case)
    B, _ = LC.reference(case, opt, vmax)
    # the run is the one tests/test_long_cases_ref.py holds the preconditions of
    assert LC.tied_to_cpu(case, opt, vmax, ((0, 1),) + case.geoms), (opt, vmax, LC.lib_options(case))
    # the census of the run the device is compared with reaches what the case is named for
    for switch, side, members in case.reach:
        sl = 0 if case.kind in ("row", "travel") else 3
        ok, v = LC.side_reached(LC.census_of(case, members, sl, opt, vmax), switch, side)
        assert ok, (case.name, switch, side, members, v)
    one = LC.census_of(case, 1, 0, opt, vmax)
    T1 = _run(c, case, 0, 1)
    _vs_ref(envelope, "%s/K1" % case.name, T1, B, steps=one.steps, close_max=int(one.hi.max()),
            accepted_max=int(one.accepted.max()), evaluated_max=int((one.ei + one.eb).max()),
            fallback_max=int(one.fallback.max()))
    failed = []
    for sl, members in ((0, 1),) + case.geoms:
        n = LC.census_of(case, members, sl, opt, vmax)
        for prof in (0, 1) if members > 1 else (1,):
            T = _run(c, case, sl, members, prof)
            if not np.array_equal(T, T1):
                failed.append(("bits", sl, members, prof, int(np.sum(T != T1))))
        got, want = _device_record(c), (LC.device_sums(n), n.steps)
        envelope["band_long/%s/record/K%d" % (case.name, members)] = {"device": got, "census": want}
        print("band_long/%s/record/K%d: device %s census %s" % (case.name, members, got, want))
        if got != want:
            failed.append(("record", sl, members, got, want))
    assert not failed, failed


@pytest.mark.parametrize("case", LC.H_CASES, ids=lambda c: c.name)
def test_row_fronts(ctx, envelope, case):
    """A full row of zero-time seeds on 6 x nx: nx cells in every list of a one-member step; nx on both
    sides of every LDS head, and the longest fronts over 2 .. 16 members of 64-, 32- and 16-column
    stripes (accepted lists on both sides of the counting sort's thresholds)."""
    _check_case(ctx, envelope, case)


@pytest.mark.parametrize("case", LC.V_CASES, ids=lambda c: c.name)
def test_column_fronts(ctx, envelope, case):
    """A full column of zero-time seeds on nz x 24 (and x 25) with 8-column stripes: the front runs
    parallel to the stripe edges, so a step has nz accepted edge cells, rim entries, claim items and
    boundary claims; two and three members."""
    _check_case(ctx, envelope, case)


@pytest.mark.parametrize("case", LC.F_CASES, ids=lambda c: c.name)
def test_fallback_rounds_and_scan(ctx, envelope, case):
    """2 n + 1 cells without a usable update() stencil in one step, on both sides of one staging round
    (128) and of the fallback list (1024, past which the cells are found by a scan); half of them in
    the first column of another member's stripe."""
    _check_case(ctx, envelope, case)


@pytest.mark.parametrize("case", LC.RAGGED_CASES, ids=lambda c: c.name)
def test_ragged_point_sources(ctx, envelope, case):
    """travel() on 1200 x 1200 grains from the centre (every list of one member past its LDS head), a
    corner and an edge midpoint; one and two members."""
    _check_case(ctx, envelope, case)


SMALL = BC.case("after_retry", "grain", (97, 129))
SMALL_SOURCE = (40, 30)


def _small_travel(c):
    veln, velpn, vm, sd = BC.model_arrays(SMALL.model, SMALL.nz, SMALL.nx)
    c.set_model(veln, velpn, vm, sd, BC.TABLE, BC.TABLE, SMALL.dnx)
    return c.travel(*[[v] for v in BC.source_xy(SMALL, SMALL_SOURCE)])[0]


def _last_error(c):
    import _alifmm

    return (_alifmm.lib().alifmm_last_error(c._h) or b"").decode()


def _capacity_case(envelope, case):
    """16 members of 8-column stripes: the first launch overflows a work list (kernel error 2), the
    call succeeds through the retry with lists 4 x as long ("cap_scale" 1 -> 4), the field is the
    reference's and the one-member run's, and the context goes on giving a fresh context's bits."""
    import _alifmm

    c, fresh = _alifmm.Context(0), _alifmm.Context(0)
    try:
        assert c.get_option("cap_scale") == 1 and fresh.get_option("cap_scale") == 1
        with pytest.raises(_alifmm.AlifmmError):
            c.set_option("cap_scale", 4)  # read-only
        opt, vmax = _set_model(c, case)
        B, _ = LC.reference(case, opt, vmax)
        assert LC.tied_to_cpu(case, opt, vmax, ((3, 16),)), (opt, vmax, LC.lib_options(case))
        n = LC.census_of(case, 16, 3, opt, vmax)
        T = _run(c, case, 3, 16, prof=1)
        scale, msg, rec = c.get_option("cap_scale"), _last_error(c), _device_record(c)
        envelope["band_long/%s/cap_scale" % case.name] = scale
        _vs_ref(envelope, "%s/K16" % case.name, T, B, steps=n.steps, cap_scale=scale)
        assert scale == 4, scale
        assert "work-list capacity 65536 exceeded" in msg, msg  # what the first launch reported
        assert rec == (LC.device_sums(n), n.steps), (rec, LC.device_sums(n), n.steps)
        assert _set_model(fresh, case) == (opt, vmax)
        T1 = _run(fresh, case, 0, 1)
        assert fresh.get_option("cap_scale") == 1  # one member holds the whole lists: no retry
        assert np.array_equal(T, T1), int(np.sum(T != T1))
        # the context after its retry: an ordinary travel, the bits of a fresh context
        assert np.array_equal(_small_travel(c), _small_travel(fresh))
        assert c.get_option("cap_scale") == 4 and fresh.get_option("cap_scale") == 1
    finally:
        c.close()
        fresh.close()


def test_capacity_loud(envelope):
    """A full column of seeds at column 3 of 3900 x 128: member 0 is handed the 7800 close cells of
    columns 2 and 4 against 4096 list entries per member: the hand-over's push reports it."""
    _capacity_case(envelope, LC.CAP_LOUD)


def test_capacity_dropped_claims(envelope):
    """1000 seeds in every third row of column 2 of 3000 x 128: member 0's step 0 claims 3000 interior
    and 2999 boundary cells, each list within the 4096 entries, their sum not: the kernel reports the
    sum (err 2 where nEb is clamped).  Before it did, step 0 dropped the 1903 boundary cells past the
    4096 without a word; measured on that kernel, the call still returned the reference's field,
    because the same launch then overflowed a list loudly (the close set is left full by that step)
    and the retry ran the whole band again: no case was found in which the drop stays silent to the
    end.  So this case pins the retry and the report, not a wrong field."""
    _capacity_case(envelope, LC.CAP_DROPPED)

