"""The band kernel's evaluation hand-out (fmm_band_k.hip, P4) at thin row-front shapes.

P4 gives every wave the chunk of 64 claimed cells at its own index and hands out every further chunk
from an LDS counter as waves come free.  A step with at most 768 claimed cells (one chunk per wave)
never touches the counter; up to 1536 cells there are at most 12 further chunks, past it some wave
takes a third; past 1792 (kEcap) the dynamic loop reads the claimed list's global form.  Which wave
evaluates a chunk cannot change a field bit: the pass reads the state of the last step's end and
writes one value per claimed cell.

Cases: a full row of zero-time seeds on 6 x nx (long_cases._h), one and two members, with member 0's
largest per-step evaluated count (ei + eb of the CPU census) within 64 below and within 64 above
each of 768, 1536 and 1792; in the two-member "over" cases the interior count is no multiple of 64
while boundary cells follow, so one chunk of the dynamic loop straddles nEi (half load_tb cells,
half load_nb cells, evaluated through load_nb).  test_census_reaches_each_side holds the census on
the CPU; the GPU test asserts it again for the options the context has in force, then the fields
bitwise against the correctly rounded CPU model and against the one-member run, with prof 0 and 1,
and with prof 1 the kernel's own sums against the census (as tests/test_gpu_band_long.py).

Measured on the MI355X when the file was written: every field bit-equal to the CPU model and to the
one-member run, every record equal to the census; the file in about 1 s.
"""
import numpy as np
import pytest

import band_cases as BC
import long_cases as LC

K_WAVE = 64
# (what the hand-out does differently past it, the evaluated count it is compared with)
THRESHOLDS = {
    "counter": LC.K_THREADS,          # nE <= 768: one static chunk per wave, the counter untouched
    "second_chunk": 2 * LC.K_THREADS,  # nE <= 1536: 12 static + at most 12 dynamic chunks
    "eval_lds": LC.K_ECAP,            # nE <= 1792: the claimed list in LDS inside the dynamic loop
}


def _case(nx, members, threshold, side):
    c = LC._h(nx, [], geoms=[(0, members)] if members > 1 else [])
    return c._replace(name="%s_K%d" % (c.name, members)), members, threshold, side


CASES = [
    _case(740, 1, "counter", "under"), _case(800, 1, "counter", "over"),
    _case(1500, 1, "second_chunk", "under"), _case(1570, 1, "second_chunk", "over"),
    _case(1760, 1, "eval_lds", "under"), _case(1830, 1, "eval_lds", "over"),
    # two members of 64-column stripes: 60 interior and 4 boundary cells per own stripe
    _case(1500, 2, "counter", "under"), _case(1560, 2, "counter", "over"),
    _case(3050, 2, "second_chunk", "under"), _case(3100, 2, "second_chunk", "over"),
    _case(3560, 2, "eval_lds", "under"), _case(3620, 2, "eval_lds", "over"),
]
IDS = [c[0].name for c in CASES]
# the two-member cases whose dynamic loop has a chunk across nEi
STRADDLE = ("h_6x1560_K2", "h_6x3100_K2", "h_6x3620_K2")


def _evaluated(n):
    return (n.ei + n.eb)[:, 0]


def _reached(n, threshold, side):
    """Member 0's largest per-step evaluated count lies in (cap - 64, cap] / (cap, cap + 64]."""
    cap, v = THRESHOLDS[threshold], int(_evaluated(n).max())
    return (cap - K_WAVE < v <= cap) if side == "under" else (cap < v <= cap + K_WAVE), v


def _straddles(n):
    """A step of member 0 inside the dynamic loop whose interior list ends inside a chunk that
    boundary cells complete."""
    ei, eb = n.ei[:, 0], n.eb[:, 0]
    return bool(((ei + eb > LC.K_THREADS) & (ei % K_WAVE != 0) & (eb > 0)).any())


def _check_census(case, members, threshold, side, opt=None, vmax=None):
    n = LC.census_of(case, members, 0, opt, vmax)
    ok, v = _reached(n, threshold, side)
    assert ok, (case.name, threshold, side, v)
    if members > 1:
        assert int(n.eb[:, 0].max()) > 0, case.name  # the list has a boundary tail
    if case.name in STRADDLE:
        assert _straddles(n), (case.name, n.ei[:, 0].tolist(), n.eb[:, 0].tolist())
    return n


@pytest.mark.parametrize("case,members,threshold,side", CASES, ids=IDS)
def test_census_reaches_each_side(case, members, threshold, side):
    """CPU only: the reference is finite and the census puts the case where it is named for."""
    F, _ = LC.reference(case)
    assert F.shape == (case.nz, case.nx) and np.isfinite(F).all() and (F >= 0).all()
    _check_census(case, members, threshold, side)


def test_every_threshold_from_both_sides():
    for members in (1, 2):
        have = {(t, s) for _, m, t, s in CASES if m == members}
        assert have == {(t, s) for t in THRESHOLDS for s in ("under", "over")}, members
    assert {c[0].name for c in CASES} >= set(STRADDLE)


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    yield c
    c.close()


BAND_OPTS = ("cdelta", "cdelta_far", "r_far", "r0", "exact_r")


def _run(c, case, members, prof):
    try:
        c.set_option("members", members)
        c.set_option("prof", prof)
        iz, ix, t = LC.seeds_of(case)
        c.travel_seeded(iz, ix, times=t, copy_out=False)
        assert c.get_option("last_k") == members
        return c.get_field(0, 1)
    finally:
        c.set_option("prof", 0)
        c.set_option("members", 0)


def _device_record(c):
    return tuple(int(v) for v in c.band_profile(0)[6:10]), int(c.source_stats(0)[0][3])


@pytest.mark.gpu
@pytest.mark.parametrize("case,members,threshold,side", CASES, ids=IDS)
def test_hand_out_keeps_the_bits(ctx, envelope, case, members, threshold, side):
    veln, velpn, vm, sd = LC.model_arrays(case)
    ctx.set_model(veln, velpn, vm, sd, BC.TABLE, BC.TABLE, LC.DNX)
    opt, vmax = {k: ctx.get_option(k) for k in BAND_OPTS}, ctx.get_option("vmax")
    geoms = ((0, 1),) + case.geoms
    assert LC.tied_to_cpu(case, opt, vmax, geoms), (opt, vmax, LC.lib_options(case))
    # the census of the run the device is compared with reaches the side the case is named for
    _check_census(case, members, threshold, side, opt, vmax)
    B, _ = LC.reference(case, opt, vmax)
    failed = []
    T1 = None
    for _, k in geoms:
        n = LC.census_of(case, k, 0, opt, vmax)
        for prof in (0, 1):
            T = _run(ctx, case, k, prof)
            T1 = T if T1 is None else T1
            bad_ref, bad_one = int(np.sum(T != B)), int(np.sum(T != T1))
            envelope["band_dispatch/%s/K%d/prof%d" % (case.name, k, prof)] = {"ne_model": bad_ref, "ne_K1": bad_one}
            print("band_dispatch/%s K%d prof %d: cells unequal to the CPU model %d, to K = 1 %d"
                  % (case.name, k, prof, bad_ref, bad_one))
            if bad_ref or bad_one:
                failed.append(("bits", k, prof, bad_ref, bad_one))
        got, want = _device_record(ctx), (LC.device_sums(n), n.steps)  # (of the prof 1 run)
        envelope["band_dispatch/%s/record/K%d" % (case.name, k)] = {"device": got, "census": want}
        print("band_dispatch/%s record K%d: device %s census %s" % (case.name, k, got, want))
        if got != want:
            failed.append(("record", k, got, want))
    assert not failed, failed
