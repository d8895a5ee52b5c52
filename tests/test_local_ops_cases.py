"""What tests/test_gpu_local_ops.py relies on, from the oracle alone (tests/local_ops_cases.py): the
designed case set reaches what it is built to reach, so the device test cannot pass emptily.  These
are conditions on the set, not measurements: a seed that misses one is changed, the condition stays."""
import numpy as np

import local_ops_cases as LC
import oracle as O

EXACT = 1e-12  # the project's bar between the glibc and the correctly rounded build (test_gpu_parity.py)


def _centre(cs, pattern, field=0):
    """Indices of the centre set's 4096 masks of one time field, in mask order."""
    sel = np.flatnonzero((cs.pattern == pattern) & (cs.field == field))
    assert len(sel) == 4096 and np.array_equal(cs.mask[sel], np.arange(4096))
    return sel


def test_update_case_set(envelope):
    sets = LC.update_sets()
    assert [s.name for s in sets] == ["update_centre", "update_cells", "update_quirk_rows", "update_quirk_bound"]
    assert 30000 <= sum(len(s.ttn) for s in sets) <= 40000
    for cs in sets:
        r = LC.reference(cs)
        assert np.all((r == -1.0) | (np.isfinite(r) & (r > 0))), cs.name
        share = float(np.mean(r == -1.0))
        envelope["local_ops_cases/%s" % cs.name] = {"cases": len(r), "share_minus1": share}
        assert 0.05 <= share <= 0.7, (cs.name, share)  # both exits of update() are well covered
        # every kind of material and every special orientation occurs
        assert len(set(cs.mat)) >= LC.NMAT - 2, cs.name
    centre, cells, rows, bound = sets
    r = LC.reference(centre)
    # the 25 positions: the centre here, the 24 others in update_cells
    assert set(zip(cells.iz, cells.ix)) == {(z, x) for z in range(5) for x in range(5)} - {(2, 2)}
    assert set(rows.nnz) == {6, 7, 8, 9} and set(rows.iz) == {3, 4} and set(rows.ix) == {0, 2, 4}
    assert rows.ttn.shape[1:] == (5, 5) and bound.ttn.shape[1:] == (7, 5)
    assert set(bound.nnz) == {5} and set(bound.nnx) == {5} and set(bound.iz) == {3, 4, 5, 6}
    # the loader's clamped reads land on valid nodes outside the operator's bounds: at the patch
    # edge a slot one column out wraps onto the neighbouring row, and in update_quirk_bound the
    # rows at and past nnz_arg hold valid nodes
    edge = np.flatnonzero(cells.ix == 0)
    wrapped = cells.nsts[edge, np.maximum(cells.iz[edge] - 1, 0), 4] >= 0  # what slot (0, -1) reads at ix = 0
    assert wrapped[cells.iz[edge] > 0].mean() > 0.5
    assert np.mean(bound.nsts[:, 5:, :] >= 0) > 0.5
    for pattern, field in ((0, 0), (1, 0), (1, 1), (2, 0), (3, 0)):
        sel = _centre(centre, pattern, field)
        assert r[sel[0]] == -1.0, (pattern, field)  # the all-invalid mask
    # each square stencil alone is enough for a value, on the all-tie field
    tie = r[_centre(centre, 1, 0)]
    single = [tie[m] for m in LC.STENCIL_MASK]
    assert all(v != -1.0 for v in single), single
    # pattern (b): the eight stencils tie in |T_a - T_b| and give eight different values, and with
    # stencils k .. 7 complete the value is stencil k's: the first minimum, strict '<', lowest index
    assert len(set(single)) == 8, single
    for k in range(8):
        m = 0
        for j in range(k, 8):
            m |= LC.STENCIL_MASK[j]
        assert tie[m] == single[k], (k, tie[m], single)
    assert len(set(tie)) >= 8
    # pattern (d): a stencil whose difference is 1e6 or more is never chosen.  The mask whose only
    # complete stencil is such a one gives what the same mask without the stencil's apex gives;
    # the two stencils just below 1e6 are chosen: stencil 1 although stencil 0 (exactly 1e6) comes
    # first, and with every slot valid stencil 5
    lim = r[_centre(centre, 3, 0)]
    t = LC.limit_field()
    slot = lambda k: t[2 + LC.SLOT_DZ[k], 2 + LC.SLOT_DX[k]]
    d = [abs(slot(LC.SA[k]) - slot(LC.SB[k])) for k in range(8)]
    assert d[0] == 1e6 and d[4] == 1e6
    assert d[1] == 1e6 - 2.0 ** -30 < 1e6 and d[5] == 1e6 - 2.0 ** -20 < 1e6
    assert all(d[k] > 1e6 for k in (2, 3, 6, 7))
    for k in (0, 2, 3, 4, 6, 7):
        m = LC.STENCIL_MASK[k]
        assert lim[m] == lim[m & ~(1 << LC.AP[k])], k
    assert lim[LC.STENCIL_MASK[1]] != -1.0 and lim[LC.STENCIL_MASK[5]] != -1.0
    assert lim[LC.STENCIL_MASK[0] | LC.STENCIL_MASK[1]] == lim[LC.STENCIL_MASK[1]]
    assert lim[4095] == lim[LC.STENCIL_MASK[5]]  # the smaller of the two differences below 1e6


def test_fouds18_case_set(envelope):
    centre, rim = LC.fouds_sets()
    assert len(centre.ttn) == 4096 and len(rim.ttn) == 1024
    assert set(zip(rim.iz, rim.ix)) == set(LC.RIM) and len(LC.RIM) == 16
    assert np.array_equal(np.unique(centre.mask), np.arange(256)) and set(centre.field) == set(range(16))
    for cs in (centre, rim):
        r = LC.reference(cs)
        assert np.all(np.isfinite(r) & (r >= 0)), cs.name
        assert set(np.unique(cs.nsts)) == {-1, 0, 1} and set(cs.pattern) == {0, 1, 2}
        cur = cs.ttn[np.arange(len(r)), cs.iz, cs.ix]
        half = float(np.mean(cur == 0.0))
        assert 0.4 <= half <= 0.6, (cs.name, half)  # both branches of the combination's `cur != 0`
        # no family has a candidate: the value is ttn[iz, ix] (0 where that is 0), in every position class
        none = r == cur
        envelope["local_ops_cases/%s" % cs.name] = {"cases": len(r), "share_no_candidate": float(none.mean())}
        for pos in sorted(set(zip(cs.iz, cs.ix))):
            at = (cs.iz == pos[0]) & (cs.ix == pos[1])
            assert np.any(none & at) and not np.all(none[at]), pos
        assert np.any(none & (cur == 0.0)) and np.any(none & (cur != 0.0)), cs.name


def test_builds_agree(golden, envelope):
    """The glibc build and the correctly rounded build of the oracle agree to 1e-12 relative on
    every case of the three input sets; the share that is bit-equal is recorded, not asserted."""
    g = golden("local_ops")
    todo = [(cs, LC.reference(cs), LC.reference(cs, O.LIB_GLIBC)) for cs in LC.update_sets() + LC.fouds_sets()]
    todo += [(cs, LC.golden_reference(g, cs), LC.golden_reference(g, cs, O.LIB_GLIBC)) for cs in LC.golden_sets(g)]
    for cs, a, b in todo:
        rel = np.abs(a - b) / np.maximum(np.abs(a), 1e-300)
        envelope["local_ops_cases/builds/%s" % cs.name] = {"bit_equal": float(np.mean(a == b)), "rel_max": float(rel.max())}
        assert rel.max() <= EXACT, (cs.name, float(rel.max()))
    # the golden vectors are the reference's own results: the glibc build reproduces them
    u, f = LC.golden_sets(g)
    assert np.array_equal(LC.golden_reference(g, u, O.LIB_GLIBC), g["u_out"])
    assert np.array_equal(LC.golden_reference(g, f, O.LIB_GLIBC), g["f_out"])
