"""The CPU side of the long-list cases (tests/long_cases.py): the preconditions of
tests/test_gpu_band_long.py.  Every reference field is finite; every case reaches, by the census, the
side of the kernel switch it is named for, so that a change of a constant or of a generator that
quietly un-reaches a regime fails here and not on the GPU; the C statement of the seeded run equals
the Python one bit for bit.
"""
import numpy as np
import pytest

import band_cases as BC
import long_cases as LC
import seed_cases as SC

PLANE = LC.H_CASES + LC.V_CASES + [LC.CAP_LOUD]


def _stripe_log(c):
    return 3 if c.kind != "row" and c.kind != "travel" else 0


@pytest.mark.parametrize("model,nz,nx", SC.MODEL_GRIDS)
def test_field_c_is_field(model, nz, nx):
    """oracle/band_model.c oband_seeded against SeedRef.field on the seeded matrix's host-time sets."""
    case = SC.case(model, nz, nx)
    o, vmax = BC.lib_options(case), BC.model_vmax(case)
    R = SC.ref_for(case)
    for s in SC.seed_sets(nz, nx, vmax):
        if s.t is None:
            continue
        F = SC.ref_field(case, s, s.t, o, vmax)
        G = R.field_c(s.iz, s.ix, s.t, vmax, o["cdelta"], o["r0"], o["cdelta_far"], o["r_far"])
        assert np.array_equal(F, G), s.name


@pytest.mark.parametrize("c", LC.ALL_DEVICE_CASES, ids=lambda c: c.name)
def test_reference_is_finite(c):
    F, log = LC.reference(c)
    assert F.shape == (c.nz, c.nx) and np.isfinite(F).all() and (F >= 0).all()
    if c.kind == "travel":
        assert int(np.sum(F == 0)) == 1 and F[c.arg[1], c.arg[0]] == 0
    else:
        iz, ix, t = LC.seeds_of(c)
        assert len(iz) + int(np.sum(log.step == -1)) <= LC.HANDOVER_MAX
        Z = F == 0
        assert int(Z.sum()) == len(iz) and Z[iz, ix].all()


@pytest.mark.parametrize("c", LC.H_CASES + LC.V_CASES + LC.F_CASES, ids=lambda c: c.name)
def test_straddles(c):
    for switch, side, members in c.reach:
        ok, v = LC.side_reached(LC.census_of(c, members, _stripe_log(c)), switch, side)
        assert ok, (c.name, switch, side, members, v)


def test_sort_windows():
    """Accepted lists in (kSortAcc, kAcap] at member counts on both sides of kSortKmax, and the 3400
    case past kAcap at two members and within kSortAcc at sixteen."""
    by = {c.name: c for c in LC.H_CASES}
    for name, members, sorts in LC.SORT_WINDOWS:
        a = LC.census_of(by[name], members, 0).accepted
        assert ((a > LC.K_SORT_ACC) & (a <= LC.K_ACAP)).any(), (name, members)
        assert (members <= LC.K_SORT_KMAX) == sorts
    assert LC.census_of(by["h_6x3400"], 2, 0).accepted.max() > LC.K_ACAP
    assert LC.census_of(by["h_6x3400"], 16, 0).accepted.max() <= LC.K_SORT_ACC
    one = LC.census_of(by["h_6x3400"], 1, 0)
    assert one.hi.max() > LC.K_LCAP and one.accepted.max() > LC.K_ACAP and (one.ei + one.eb).max() > LC.K_ECAP


def test_v_family_last_stripe_of_one_column():
    c = [v for v in LC.V_CASES if v.nx == 25][0]
    n = LC.census_of(c, 3, 3)
    # stripe 3 is column 24 alone: member 0's; its cells are EDGE and RIM cells, all claimed from column 23's rim items
    assert n.rx[:, 0].max() > LC.K_THREADS and n.eb[:, 0].max() > LC.K_BCAP


def test_ragged_reaches_the_spill_sides():
    centre = LC.RAGGED_CASES[0]
    one, two = LC.census_of(centre, 1, 0), LC.census_of(centre, 2, 0)
    assert one.hi.max() > LC.K_LCAP and one.accepted.max() > LC.K_ACAP and (one.ei + one.eb).max() > LC.K_ECAP
    # two members: the close set and the evaluation in LDS, their sum past the LDS commit
    assert two.hi.max() <= LC.K_LCAP and (two.ei + two.eb).max() <= LC.K_ECAP
    assert (two.hi + two.ei + two.eb).max() > LC.K_LCAP
    for c in LC.RAGGED_CASES[1:]:
        n = LC.census_of(c, 1, 0)
        assert n.hi.max() <= LC.K_LCAP and LC.K_SORT_ACC < n.accepted.max() <= LC.K_ACAP


def test_fallback_and_tile_counts_of_the_point_sources():
    """No point-source case has a step with more than one fallback cell (a second staging round
    needs 128, the scan 1024: the F cases reach them), nor a member completing more than
    ts::kListCap tiles in a step: the largest counts found are recorded.  The
    plane fronts have no fallback cell after the seed step."""
    fb = tiles = 0
    for c in LC.RAGGED_CASES + [LC.MIXED_CENSUS_CASE]:
        for members in (1, 2):
            n = LC.census_of(c, members, 0, tiles=True)
            fb, tiles = max(fb, int(n.fallback.max())), max(tiles, int(n.tiles.max()))
    for c in PLANE:
        for sl, members in ((0, 1),) + c.geoms:
            assert LC.census_of(c, members, sl).fallback.max() == 0, c.name
    assert (fb, tiles) == (LC.FALLBACK_MOST, LC.TILES_MOST)
    assert fb <= LC.K_FB_ROUND and tiles <= LC.TS_LIST_CAP


def test_capacity_cases():
    loud = LC.census_of(LC.CAP_LOUD, 16, 3)
    assert loud.close[0, 0] == 2 * LC.CAP_LOUD.nz > LC.CAP_PER_MEMBER and (loud.close[0, 1:] == 0).all()
    assert LC.CAP_LOUD.nz * LC.CAP_LOUD.nx // 8 <= 65536  # the lists' floor: 65536 / 16 per member
    assert max(loud.hi.max(), (loud.ei + loud.eb).max()) <= 4 * LC.CAP_PER_MEMBER  # fits after one retry
    d = LC.census_of(LC.CAP_DROPPED, 16, 3)
    assert d.close[0, 0] == 3999 <= LC.CAP_PER_MEMBER and d.accepted[0, 0] == 3999
    assert (d.ei[0, 0], d.eb[0, 0]) == (3000, 2999)
    assert d.ei[0, 0] <= LC.CAP_PER_MEMBER and d.eb[0, 0] <= LC.CAP_PER_MEMBER < d.ei[0, 0] + d.eb[0, 0]
    assert max(d.hi.max(), (d.ei + d.eb).max()) <= 4 * LC.CAP_PER_MEMBER
    assert d.fallback[0, 0] == 2001  # after the retry the run also takes the fallback's scan


@pytest.mark.parametrize("c", [LC.H_CASES[-2], LC.V_CASES[-1], LC.RAGGED_CASES[1]], ids=lambda c: c.name)
def test_census_totals_do_not_depend_on_the_members(c):
    F, log = LC.reference(c)
    one = LC.census_of(c, 1, 0)
    assert one.accepted.sum() == int(np.sum(log.acc >= 0)) and (one.ei + one.eb).sum() == int(np.sum(log.step >= 0))
    assert one.close[-1, 0] == one.accepted[-1, 0] and (one.eb == 0).all() and (one.rx == 0).all()
    for sl, members in c.geoms:
        n = LC.census_of(c, members, sl)
        assert n.steps == one.steps
        for f in ("close", "accepted", "fresh", "fallback"):
            assert np.array_equal(getattr(n, f).sum(1), getattr(one, f)[:, 0]), (members, f)
        assert np.array_equal((n.ei + n.eb).sum(1), one.ei[:, 0])
        # every claim item is one accepted RIM cell, and every RIM cell was published before it was accepted
        assert 0 < n.rx.sum() <= n.accepted.sum() and n.rx.sum() <= n.rim.sum()
