"""tests/seed_ref.py, the CPU statement of alifmm_travel_seeded: the preconditions of the device
test (tests/test_gpu_seeded.py holds the device to 1e-9 relative over all cells, which needs a
positive finite denominator away from zero-time seeds) and the documented properties of the one-
and two-layer starts (include/alifmm.h, alifmm_travel_seeded term 9)."""
import numpy as np
import pytest

import band_cases as BC
import seed_cases as SC


def _opt(c):
    return BC.lib_options(c)


def _times(c, s):
    if s.t is not None:
        return s.t
    return SC.incident_times(c, s, BC.model_field(c, SC.INCIDENT(c.nz, c.nx)))


def _check(c, s):
    t = _times(c, s)
    F = SC.ref_field(c, s, t, _opt(c), BC.model_vmax(c))
    assert np.isfinite(F).all(), (c.name, s.name)
    assert np.array_equal(F[s.iz, s.ix], t), (c.name, s.name)  # Dirichlet: bit for bit
    off = np.ones(F.shape, dtype=bool)
    off[s.iz[t == 0], s.ix[t == 0]] = False
    assert (F[off] > 0).all(), (c.name, s.name, float(F[off].min()))
    return F


@pytest.mark.parametrize("model,nz,nx", SC.MODEL_GRIDS)
def test_matrix_is_finite_and_positive(model, nz, nx):
    c = SC.case(model, nz, nx)
    for s in SC.seed_sets(nz, nx, BC.model_vmax(c)):
        _check(c, s)


def test_checkerboard_and_far_band_are_finite_and_positive():
    c = SC.case(*SC.CHECKER_FITS)
    s = SC.checkerboard(c.nz, c.nx, BC.model_vmax(c))
    assert len(s.iz) == 5917
    _check(c, s)
    f = BC.case("seed_far", SC.FAR_GRID[0], SC.FAR_GRID[1:], opts=SC.FAR_OPTS, dnx=SC.DNX)
    s = SC.seed_sets(f.nz, f.nx, BC.model_vmax(f))[0]
    F = _check(f, s)
    off = BC.case("seed_far_off", SC.FAR_GRID[0], SC.FAR_GRID[1:], opts={"cdelta_far": 0.0}, dnx=SC.DNX)
    G = SC.ref_field(off, s, s.t, _opt(off), BC.model_vmax(off))
    assert int(np.sum(F != G)) > 1000  # the far band is engaged: it changes the field


def test_two_layers_continue_a_plane_front_exactly():
    c = SC.case("iso", 41, 127)
    v = BC.model_vmax(c)
    s = SC.seed_sets(c.nz, c.nx, v)[3]
    assert s.name == "two_layers"
    F = SC.ref_field(c, s, s.t, _opt(c), v)
    want = (np.arange(c.nz) * c.dnz / v)[:, None] * np.ones((1, c.nx))
    rel = np.abs(F[1:] - want[1:]) / want[1:]
    print("two layers: rel max %.3e" % rel.max())
    assert rel.max() <= 1e-12


def test_one_layer_starts_a_third_of_a_cell_early():
    c = SC.case("iso", 41, 127)
    v = BC.model_vmax(c)
    s = SC.seed_sets(c.nz, c.nx, v)[0]
    assert s.name == "top0"
    F = SC.ref_field(c, s, s.t, _opt(c), v)
    inner, side = (2.0 / 3.0) * c.dnz / v, c.dnz / v
    rel = np.abs(F[1, 1:-1] - inner) / inner
    print("one layer: rel max %.3e, side columns %.6e %.6e (dnz / v %.6e)" % (rel.max(), F[1, 0], F[1, -1], side))
    assert rel.max() <= 1e-9
    assert abs(F[1, 0] - side) <= 1e-9 * side and abs(F[1, -1] - side) <= 1e-9 * side
