"""Reuse of source-init hand-overs (option "init_reuse", csrc/fmm_shared.h InitSig): a source whose
walk would read what the walk that filled its slot read is not walked again, and nothing else is.

Every case compares with a fresh context on the same model with init_reuse 0 (every source walked,
no signature kept), bit for bit, at subgrid 1, on a 64 x 160 anisotropic model of four materials
and on a table-velocity model.  W = max(exact_r + 6, 16) = 26 cells is the reach of a signature's
window (csrc/init_sig.h)."""
import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu

NZ, NX, DNX = 64, 160, 1e-3
REACH = 26  # exact_r 20 (the default) + 6


def aniso_model():
    """Stiffness velocities (velpn 0), four (orientation, scale) materials in blocks."""
    veln = np.zeros((NZ, NX))
    veln[:, 50:110] = 30.0
    veln[:, 110:] = 65.0
    veln[40:, 20:90] = 120.0
    vm = np.ones((NZ, NX))
    vm[:, 110:] = 0.97
    return veln, np.zeros((NZ, NX), dtype=np.int64), vm, W.stif_field(NZ, NX)


def table_model():
    """Table velocities (velpn 1, no stiffness), two scales; the table's column 1 varies with angle."""
    veln = np.zeros((NZ, NX))
    veln[:, 70:] = 40.0
    vm = 5790.0 * np.ones((NZ, NX))
    vm[30:, :] = 5200.0
    return veln, np.ones((NZ, NX), dtype=np.int64), vm, None


def table():
    t = W.default_table()
    t[:, 1] = 1.0 + 0.1 * np.cos(np.deg2rad(2.0 * t[:, 0]))
    return t


MODELS = {"aniso": (aniso_model, W.default_table), "table": (table_model, table)}

# corner (0, 0), top edge, interior, right edge, bottom-right corner: (x, z) nodes
FIVE = [(0, 0), (80, 0), (70, 30), (NX - 1, 32), (NX - 1, NZ - 1)]
TOP2 = [(30, 0), (120, 0)]


def _xz(nodes, dnx=DNX):
    a = np.array(nodes, dtype=np.float64)
    return dnx * a[:, 0], dnx * a[:, 1]


def _ctx(model, vt, dnx=DNX, **opts):
    import _alifmm

    c = _alifmm.Context(0)
    for k, v in opts.items():
        c.set_option(k, v)
    c.set_model(*model, vt, vt, dnx)
    return c


def fresh(model, vt, nodes, dnx=DNX, subgrid=1, **opts):
    """The reference: a new context, every source walked."""
    c = _ctx(model, vt, dnx, init_reuse=0, **opts)
    try:
        F = c.travel(*_xz(nodes, dnx), subgrid=subgrid)
        assert c.get_option("init_reused") == 0
        return F
    finally:
        c.close()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope="module")
def ref_five():
    """Fresh fields of FIVE on both models, shared (read only)."""
    out = {}
    for name, (mk, tab) in MODELS.items():
        out[name] = fresh(mk(), tab(), FIVE)
        out[name].setflags(write=False)
    return out


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("batch", [256, 2])  # one init launch per chunk; one per call (nsrc > chunk)
def test_same_call_twice(name, batch, ref_five):
    mk, tab = MODELS[name]
    c = _ctx(mk(), tab(), batch=batch)
    try:
        assert c.get_option("init_reuse") == 1
        F1 = c.travel(*_xz(FIVE))
        assert c.get_option("init_reused") == 0
        F2 = c.travel(*_xz(FIVE))
        assert c.get_option("init_reused") == 5
        assert same_bits(F1, ref_five[name]) and same_bits(F2, ref_five[name])
        c.set_option("init_reuse", 0)
        F3 = c.travel(*_xz(FIVE))
        assert c.get_option("init_reused") == 0
        assert same_bits(F3, ref_five[name])
        # back on: the slots were left without a valid signature, so one walk, then reuse
        c.set_option("init_reuse", 1)
        F4 = c.travel(*_xz(FIVE))
        assert c.get_option("init_reused") == 0
        F5 = c.travel(*_xz(FIVE))
        assert c.get_option("init_reused") == 5
        assert same_bits(F4, ref_five[name]) and same_bits(F5, ref_five[name])
    finally:
        c.close()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_window_boundaries(name):
    mk, tab = MODELS[name]
    vt = tab()
    base = mk()
    (x0, z0), _ = TOP2

    def edited(z, x):
        m = tuple(None if a is None else a.copy() for a in base)
        m[0][z, x] += 17.0  # orientation
        return m

    inside = edited(z0 + REACH, x0 + REACH)   # the last cell inside the first source's window
    outside = edited(z0 + REACH + 1, x0)      # one row past it: outside every window
    c = _ctx(base, vt)
    try:
        c.travel(*_xz(TOP2), copy_out=False)
        c.set_model(*inside, vt, vt, DNX)
        F = c.travel(*_xz(TOP2))
        assert c.get_option("init_reused") == 1
        assert same_bits(F, fresh(inside, vt, TOP2))
        c.set_model(*base, vt, vt, DNX)
        c.travel(*_xz(TOP2), copy_out=False)
        assert c.get_option("init_reused") == 1  # the first source's window went back
        c.set_model(*outside, vt, vt, DNX)
        F = c.travel(*_xz(TOP2))
        assert c.get_option("init_reused") == 2
        R = fresh(outside, vt, TOP2)
        assert same_bits(F, R)
        assert not same_bits(R, fresh(base, vt, TOP2))  # (the edit does reach the fields)
    finally:
        c.close()


THREE = TOP2 + [(70, 30)]
FAR = (60, 150)  # (z, x): more than REACH from every source of THREE


def _copy(m):
    return tuple(None if a is None else a.copy() for a in m)


def _inval_dnx():
    m, vt = aniso_model(), W.default_table()
    return (m, vt, DNX, {}), (m, vt, 2 * DNX, {})


def _inval_exact_r():
    m, vt = aniso_model(), W.default_table()
    return (m, vt, DNX, {}), (m, vt, DNX, {"exact_r": 12})


def _inval_table():
    m, vt = table_model(), table()
    vt2 = vt.copy()
    vt2[100, 1] *= 0.999  # one entry (not the column's maximum: vmax stays)
    return (m, vt, DNX, {}), (m, vt2, DNX, {})


def _inval_stiffness():
    m, vt = aniso_model(), W.default_table()
    m2 = _copy(m)
    m2[3][FAR[0], FAR[1], 3] += 1000  # one value of one far cell: another stiffness row
    return (m, vt, DNX, {}), (m2, vt, DNX, {})


def _inval_vmax():
    m, vt = aniso_model(), W.default_table()
    m2 = _copy(m)
    m2[2][FAR] = 1.5  # a far cell faster than the rest: vmax, so tstop
    return (m, vt, DNX, {}), (m2, vt, DNX, {})


@pytest.mark.parametrize("case", [_inval_dnx, _inval_exact_r, _inval_table, _inval_stiffness, _inval_vmax],
                         ids=lambda f: f.__name__[7:])
def test_whole_call_invalidation(case):
    (m1, vt1, d1, o1), (m2, vt2, d2, o2) = case()
    c = _ctx(m1, vt1, d1, **o1)
    try:
        c.travel(*_xz(THREE, d1), copy_out=False)
        c.travel(*_xz(THREE, d1), copy_out=False)
        assert c.get_option("init_reused") == 3
        for k, v in o2.items():
            c.set_option(k, v)
        c.set_model(*m2, vt2, vt2, d2)
        F = c.travel(*_xz(THREE, d2))
        assert c.get_option("init_reused") == 0
        assert same_bits(F, fresh(m2, vt2, THREE, d2, **o2))
    finally:
        c.close()


def test_slots_and_arena(ref_five):
    mk, tab = MODELS["aniso"]
    m, vt = mk(), tab()
    c = _ctx(m, vt)
    try:
        # swapped order: only the middle source finds its own hand-over in its slot
        c.travel(*_xz(THREE), copy_out=False)
        F = c.travel(*_xz(THREE[::-1]))
        assert c.get_option("init_reused") == 1
        assert same_bits(F, fresh(m, vt, THREE[::-1]))
        # a larger batch, then a smaller one of other sources in the same slots
        assert same_bits(c.travel(*_xz(FIVE)), ref_five["aniso"])
        small = [FIVE[3], FIVE[2]]
        F = c.travel(*_xz(small))
        assert c.get_option("init_reused") == 0
        assert same_bits(F, fresh(m, vt, small))
        # a subgrid 3 call in between
        c.travel(*_xz(FIVE), copy_out=False)
        F3 = c.travel(*_xz(THREE), subgrid=3)
        assert c.get_option("init_reused") == 0
        assert same_bits(F3, fresh(m, vt, THREE, subgrid=3))
        assert same_bits(c.travel(*_xz(FIVE)), ref_five["aniso"])
    finally:
        c.close()


@pytest.mark.parametrize("members", [1, 2, 4])
def test_working_arena_between_calls(members):
    """A source set, then a disjoint one of the same size on the same context (a cell of the
    working field left from the first would read as valid in the second), and a call on another
    grid size in between."""
    mk, tab = MODELS["aniso"]
    m, vt = mk(), tab()
    s1 = [(10, 0), (100, 0), (40, 63)]
    s2 = [(150, 20), (60, 40), (0, 63)]
    geom = {"members": members, "stripe_log": 4}  # ten 16-column stripes: room for four members
    r2 = fresh(m, vt, s2, **geom)
    c = _ctx(m, vt, **geom)
    try:
        c.travel(*_xz(s1), copy_out=False)
        assert c.get_option("last_k") == members
        assert same_bits(c.travel(*_xz(s2)), r2)
        c.travel(*_xz(s1), copy_out=False)
        other = tuple(None if a is None else np.ascontiguousarray(a[:40, :96]) for a in m)
        c.set_model(*other, vt, vt, DNX)
        c.travel(*_xz([(10, 0), (90, 39), (50, 20)]), copy_out=False)
        c.set_model(*m, vt, vt, DNX)
        assert same_bits(c.travel(*_xz(s2)), r2)
    finally:
        c.close()
