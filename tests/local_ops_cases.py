"""The designed case set of the two local operators, update() and fouds18_A(), shared by
tests/test_local_ops_cases.py (the oracle's side: the set reaches what it is meant to reach) and
tests/test_gpu_local_ops.py (the device's side: every form of the operators in csrc/local_ops.h
equals the correctly rounded oracle build bit for bit).

Everything is seeded numpy, built once per process.  A set is a batch of independent patches with
the operator's arguments and one material record per case; the reference values of a set come from
oracle.open_lib(build)'s oref_update / oref_fouds18 and are cached per (set, build).

update() slots (fields.h NbField::slot), bit k of a case's mask = slot k valid:
  0..3 (0, -2) (0, -1) (0, 1) (0, 2);  4..7 (-2, 0) (-1, 0) (1, 0) (2, 0);  8..11 (-1, -1) (-1, 1) (1, -1) (1, 1)
Square stencil k reads its apex AP[k] and the pair SA[k], SB[k] (local_ops.h update_nb_select).
"""
import collections

import numpy as np

import oracle as O

SLOT_DZ = np.array([0, 0, 0, 0, -2, -1, 1, 2, -1, -1, 1, 1])
SLOT_DX = np.array([-2, -1, 1, 2, 0, 0, 0, 0, -1, 1, -1, 1])
AP = (4, 3, 7, 0, 8, 9, 11, 10)
SA = (8, 9, 10, 8, 1, 5, 6, 1)
SB = (9, 11, 11, 10, 5, 2, 2, 6)
STENCIL_MASK = tuple((1 << AP[k]) | (1 << SA[k]) | (1 << SB[k]) for k in range(8))

PATTERNS = ("plane", "ties", "unordered", "limit")  # (a) .. (d)


def _tables():
    """Phase and group tables, three positive columns each (column 0 is read by velpn 0 without
    stiffness, 1 and 2 by velpn 1 and 2); row 360 closes the circle like the reference's tables."""
    a = np.deg2rad(np.arange(361.0))
    p = np.stack([5200.0 + 450.0 * np.cos(2 * a) + 60.0 * np.cos(4 * a), np.ones(361),
                  3100.0 + 280.0 * np.sin(a) ** 2 - 90.0 * np.sin(2 * a) ** 2], axis=1)
    g = np.stack([5200.0 + 380.0 * np.cos(2 * a) - 120.0 * np.cos(4 * a), np.ones(361),
                  3100.0 + 310.0 * np.sin(a) ** 2 + 140.0 * np.sin(2 * a) ** 2], axis=1)
    return np.ascontiguousarray(p), np.ascontiguousarray(g)


TAB_P, TAB_G = _tables()

# ---- materials, cycled over the cases ---------------------------------------------------------
# kind 0: velpn 0 with stiffness (Christoffel); 1: velpn 0 without stiffness (table column 0);
# 2, 3: velpn 1, 2 (table columns).  Orientations: the exact multiples of 90 and 180 and values
# within 0.005 of them (the on-axis snap of the Christoffel group velocity, pymod's wrap), then
# random ones in [-50, 400].
NMAT = 61  # prime: the cycle does not lock onto the masks' or the patterns' periods
_SPECIAL_VELN = (0.0, 90.0, 180.0, 270.0, 360.0, -0.0, 0.004, -0.004, 89.996, 90.0049, 179.9951, 180.003, 269.999,
                 270.0045, 359.9975, 360.002, 45.0, 27.0, -27.0, 135.0, 44.997, 153.002, 63.004, 333.0)

Mats = collections.namedtuple("Mats", "veln velpn vm stif_on stif")


def _materials():
    rng = np.random.default_rng(20240611)
    veln = np.empty(NMAT)
    veln[:len(_SPECIAL_VELN)] = _SPECIAL_VELN
    veln[len(_SPECIAL_VELN):] = rng.uniform(-50, 400, NMAT - len(_SPECIAL_VELN))
    # the kinds run against the orientations with a different period, so every special orientation
    # meets a Christoffel record within a few cycles of the case index
    kind = (np.arange(NMAT) * 3) % 4
    velpn = np.where(kind >= 2, kind - 1, 0).astype(np.int64)
    stif_on = kind != 1
    vm = np.where(np.arange(NMAT) % 2 == 0, 1.0, rng.uniform(0.5, 2.0, NMAT))
    stif = np.stack([rng.integers(200000, 300000, NMAT), rng.integers(100000, 150000, NMAT),
                     rng.integers(150000, 240000, NMAT), rng.integers(80000, 130000, NMAT),
                     rng.integers(7000, 9000, NMAT)], axis=1).astype(np.int64)
    stif[0] = (249000, 133000, 205000, 125000, 7850)
    return Mats(veln, velpn, vm, stif_on, stif)


MATS = _materials()
TIE_MAT = 28   # the one record of the all-tie field: Christoffel at a random orientation, so every
               # stencil's direction gives its own value
LIMIT_MAT = 25  # and of the limit field: table column 2, a random orientation

# A batch of cases of one operator on (pz, px) patches.  mat: index into MATS per case; pos / mask /
# pattern / field: what a mismatch report prints.
CaseSet = collections.namedtuple("CaseSet", "name op ttn nsts iz ix dnx nnz nnx mat mask pattern field")

Q = 2.0 ** -24  # the quantum of pattern (b): every time is a small integer multiple, differences exact


def _plane(rng, n, pz, px, dnx):
    th = rng.uniform(0, 2 * np.pi, n)
    step = dnx / 5000.0 * rng.uniform(0.5, 2.0, n)
    zz, xx = np.mgrid[0:pz, 0:px]
    t = (zz[None] * np.cos(th)[:, None, None] + xx[None] * np.sin(th)[:, None, None] + 2.0 * (pz + px))
    t = t * step[:, None, None] + rng.normal(0, 1, (n, pz, px)) * (step * 10 ** rng.uniform(-6, -2, n))[:, None, None]
    return np.abs(t) + 1e-300


def _ties(rng, n, pz, px):
    return (8 + rng.integers(0, 4, (n, pz, px))) * Q


def _unordered(rng, n, pz, px, dnx):
    return rng.uniform(0.5, 1.5, (n, pz, px)) * (dnx / 500.0)[:, None, None]


def _put_slots(field, vals, cz=2, cx=2):
    for k, v in enumerate(vals):
        field[cz + SLOT_DZ[k], cx + SLOT_DX[k]] = v


def all_tie_field():
    """Pattern (b), field 0: |T_a - T_b| is one quantum in all eight square stencils, so the first
    complete one wins (strict '<', lowest index)."""
    f = np.full((5, 5), 7 * Q)
    #            slot 0      1      2       3      4      5      6      7      8      9      10     11
    _put_slots(f, (4 * Q, 9 * Q, 11 * Q, 6 * Q, 5 * Q, 10 * Q, 10 * Q, 7 * Q, 8 * Q, 9 * Q, 9 * Q, 8 * Q))
    return f


def limit_field():
    """Pattern (d): differences around min_diff's start value 1e6.  Stencils 0 and 4: exactly 1e6;
    1 and 5: just below it; 2, 3, 6, 7: above.  Only 1 and 5 can ever be chosen."""
    f = np.full((5, 5), 3.0)
    e1, e2 = 2.0 ** -30, 2.0 ** -20
    _put_slots(f, (0.5, 2.0, 2.0 + e2, 0.75, 0.25, 2.0 + 1e6, 2.0 + 2e6, 0.625, 1.0, 1.0 + 1e6, 1.0 + 3e6, 1.0 + e1))
    return f


def _status(rng, valid):
    """-1 where invalid, 0 (known) or 3 (close) where valid."""
    return np.where(valid, rng.choice(np.array([0, 3], dtype=np.int32), valid.shape), -1).astype(np.int32)


def _mask_of(valid, iz, ix):
    """The 12-bit slot mask of cell (iz, ix) in each (pz, px) validity patch (slots inside the patch)."""
    n, pz, px = valid.shape
    m = np.zeros(n, dtype=np.int64)
    for k in range(12):
        z, x = iz + SLOT_DZ[k], ix + SLOT_DX[k]
        ok = (z >= 0) & (z < pz) & (x >= 0) & (x < px)
        m |= (ok & valid[np.arange(n), np.clip(z, 0, pz - 1), np.clip(x, 0, px - 1)]).astype(np.int64) << k
    return m


def _update_centre():
    """The centre cell of 5 x 5 patches with nnz = nnx = 5: all 4096 validity masks of the 12 slots,
    with (a) one plane front per mask, (b) the all-tie field and one seeded quantised field, (c) one
    unordered field per mask, (d) the limit field."""
    rng = np.random.default_rng(1001)
    masks = np.arange(4096)
    parts = []
    for pattern, field in ((0, 0), (1, 0), (1, 1), (2, 0), (3, 0)):
        n = 4096
        dnx = 10 ** rng.uniform(-5, -3, n)
        if pattern == 0:
            t = _plane(rng, n, 5, 5, dnx)
        elif pattern == 1:
            t = np.broadcast_to(all_tie_field() if field == 0 else _ties(rng, 1, 5, 5)[0], (n, 5, 5)).copy()
        elif pattern == 2:
            t = _unordered(rng, n, 5, 5, dnx)
        else:
            t = np.broadcast_to(limit_field(), (n, 5, 5)).copy()
        valid = rng.random((n, 5, 5)) < 0.7  # the 13 cells update() never reads
        for k in range(12):
            valid[:, 2 + SLOT_DZ[k], 2 + SLOT_DX[k]] = (masks >> k) & 1
        parts.append((t, _status(rng, valid), masks, np.full(n, pattern), np.full(n, field)))
    ttn, nsts, mask, pattern, field = (np.concatenate([p[i] for p in parts]) for i in range(5))
    n = len(ttn)
    mat = np.arange(n) % NMAT
    dnx = 10 ** np.random.default_rng(1002).uniform(-5, -3, n)
    # the two designed fields keep one record and one spacing over their masks, so that two masks'
    # results differ by the selection alone
    one = ((pattern == 1) & (field == 0)) | (pattern == 3)
    mat[(pattern == 1) & (field == 0)] = TIE_MAT
    mat[pattern == 3] = LIMIT_MAT
    dnx[one] = 1e-4
    five = np.full(n, 5, dtype=np.int32)
    return CaseSet("update_centre", 0, ttn, nsts, np.full(n, 2, np.int32), np.full(n, 2, np.int32), dnx, five, five,
                   mat, mask, pattern, field)


def _update_cells(name, seed, pz, px, cells, nnz_values, per, valid_p=0.7):
    """`per` seeded validity patches at each cell of `cells` and each nnz_arg of `nnz_values`, with
    patterns (a) and (b).  Every cell of the patch draws its own validity, so a slot outside the
    operator's bounds holds a valid value wherever the loader's clamped read lands on a valid node."""
    rng = np.random.default_rng(seed)
    iz, ix, nnz, pattern = [], [], [], []
    for (z, x) in cells:
        for nz_arg in nnz_values:
            for pat in (0, 1):
                iz += [z] * per
                ix += [x] * per
                nnz += [nz_arg] * per
                pattern += [pat] * per
    iz, ix, nnz, pattern = (np.array(v, dtype=np.int32) for v in (iz, ix, nnz, pattern))
    n = len(iz)
    dnx = 10 ** rng.uniform(-5, -3, n)
    ttn = np.where((pattern == 0)[:, None, None], _plane(rng, n, pz, px, dnx), _ties(rng, n, pz, px))
    valid = rng.random((n, pz, px)) < valid_p
    return CaseSet(name, 0, ttn, _status(rng, valid), iz, ix, dnx, nnz, np.full(n, px, np.int32), np.arange(n) % NMAT,
                   _mask_of(valid, iz, ix), pattern.astype(np.int64), np.zeros(n, dtype=np.int64))


def _build_update_sets():
    others = [(z, x) for z in range(5) for x in range(5) if (z, x) != (2, 2)]
    return [
        _update_centre(),
        # the other 24 positions reach every combination of l1 l2 r1 r2 u1 u2 d1 d2
        _update_cells("update_cells", 2001, 5, 5, others, (5,), 256),
        # the stage-1 quirk, bound past the array: nnz_arg 6 .. 9 on 5 rows (rows past it read -1 / 0)
        _update_cells("update_quirk_rows", 2002, 5, 5, [(z, x) for z in (3, 4) for x in (0, 2, 4)], (6, 7, 8, 9), 32,
                      valid_p=0.8),
        # the stage-1 quirk, array past the bound: 7 rows under nnz_arg = nnx_arg = 5, so the cells of
        # rows 4 .. 6 lie at or past update()'s bound with valid nodes below them
        _update_cells("update_quirk_bound", 2003, 7, 5, [(z, x) for z in (3, 4, 5, 6) for x in range(5)], (5,), 64,
                      valid_p=0.8),
    ]


NEAR8 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
RIM = tuple((z, x) for z in (0, 1, 5, 6) for x in (0, 1, 5, 6))


def _fouds_times(rng, n, dnx, pattern):
    t = np.empty((n, 7, 7))
    for p, make in ((0, lambda m: _plane(rng, m, 7, 7, dnx[pattern == 0])), (1, lambda m: _ties(rng, m, 7, 7)),
                    (2, lambda m: _unordered(rng, m, 7, 7, dnx[pattern == 2]))):
        sel = pattern == p
        if sel.any():
            t[sel] = make(int(sel.sum()))
    return t


def _build_fouds_sets():
    """7 x 7 patches, status in {-1, 0, 1}, nnz = nnx = 7."""
    rng = np.random.default_rng(3001)
    # the centre cell: all 2^8 known-masks of the 8 nearest nodes x 16 fillings of the outer ring
    n = 256 * 16
    mask = np.repeat(np.arange(256), 16)
    fill = np.tile(np.arange(16), 256)
    pattern = fill % 3
    dnx = 10 ** rng.uniform(-5, -3, n)
    ring_st = rng.choice(np.array([-1, 0, 1], dtype=np.int32), (16, 7, 7), p=[0.3, 0.5, 0.2])
    ring_st[0] = -1  # filling 0: nothing known outside the 8 nearest nodes
    ring_st[1] = 0   # filling 1: everything known
    nsts = ring_st[fill].copy()
    unknown = rng.choice(np.array([-1, 1], dtype=np.int32), (n, 8))
    for b, (dz, dx) in enumerate(NEAR8):
        nsts[:, 3 + dz, 3 + dx] = np.where((mask >> b) & 1, 0, unknown[:, b])
    ttn = _fouds_times(rng, n, dnx, pattern)
    cur0 = ((mask + fill) % 2) == 0
    ttn[cur0, 3, 3] = 0.0
    nsts[:, 3, 3] = 1
    seven = np.full(n, 7, np.int32)
    centre = CaseSet("fouds18_centre", 1, ttn, nsts, np.full(n, 3, np.int32), np.full(n, 3, np.int32), dnx, seven, seven,
                     np.arange(n) % NMAT, mask.astype(np.int64), pattern.astype(np.int64), fill.astype(np.int64))
    # 64 seeded cases at each of the 16 cells whose row or column is at or next to the edge
    per = 64
    n = per * len(RIM)
    iz = np.repeat(np.array([c[0] for c in RIM], dtype=np.int32), per)
    ix = np.repeat(np.array([c[1] for c in RIM], dtype=np.int32), per)
    k = np.tile(np.arange(per), len(RIM))
    pattern = k % 3
    dnx = 10 ** rng.uniform(-5, -3, n)
    nsts = rng.choice(np.array([-1, 0, 1], dtype=np.int32), (n, 7, 7), p=[0.3, 0.5, 0.2])
    nsts[k == 0] = -1  # nothing known: no family has a candidate
    ttn = _fouds_times(rng, n, dnx, pattern)
    cur0 = (k % 2) == 1
    ttn[cur0, iz[cur0], ix[cur0]] = 0.0
    seven = np.full(n, 7, np.int32)
    rim = CaseSet("fouds18_rim", 1, ttn, nsts, iz, ix, dnx, seven, seven, (np.arange(n) * 7) % NMAT,
                  np.zeros(n, dtype=np.int64), pattern.astype(np.int64), k.astype(np.int64))
    return [centre, rim]


_sets = {}


def update_sets():
    if "u" not in _sets:
        _sets["u"] = _build_update_sets()
    return _sets["u"]


def fouds_sets():
    if "f" not in _sets:
        _sets["f"] = _build_fouds_sets()
    return _sets["f"]


def all_fouds():
    """The fouds18_A() cases as one batch (the PRE_ONLY forms take their material from a resident
    model's cells instead of MATS)."""
    if "fall" not in _sets:
        s = fouds_sets()
        cat = lambda f: np.concatenate([getattr(c, f) for c in s])
        _sets["fall"] = CaseSet("fouds18_all", 1, *[cat(f) for f in CaseSet._fields[2:]])
    return _sets["fall"]


# ---- the material of a case, as the library and the oracle take it ------------------------------
def case_mats(cs):
    m = cs.mat
    return MATS.veln[m], MATS.velpn[m], MATS.vm[m], MATS.stif_on[m], MATS.stif[m]


def table(cs):
    return TAB_P if cs.op == 0 else TAB_G


def describe(cs, k):
    veln, velpn, vm, son, stif = (a[k] for a in case_mats(cs))
    return ("%s[%d] cell (%d, %d) nnz %d nnx %d mask 0x%03x pattern %s field %d dnx %.17g material veln %.17g velpn %d "
            "vm %.17g stif %s" % (cs.name, k, cs.iz[k], cs.ix[k], cs.nnz[k], cs.nnx[k], cs.mask[k],
                                  PATTERNS[cs.pattern[k]], cs.field[k], cs.dnx[k], veln, velpn, vm,
                                  list(stif) if son else None))


# ---- reference values ---------------------------------------------------------------------------
_refs = {}


def oracle_values(op, build, ttn, nsts, iz, ix, dnx, nnz, nnx, veln, velpn, vm, stif_on, stif, tab):
    """oref_update (op 0) / oref_fouds18 (op 1) of every case; the operators read the material at the
    target cell only, so each case's record fills its patch."""
    L = O.open_lib(build)
    n, pz, px = ttn.shape
    pn = pz * px
    ttn = np.ascontiguousarray(ttn, dtype=np.float64)
    nsts = np.ascontiguousarray(nsts, dtype=np.int32)
    A = np.ascontiguousarray(np.repeat(np.asarray(veln, dtype=np.float64), pn))
    B = np.ascontiguousarray(np.repeat(np.asarray(velpn, dtype=np.int64), pn))
    C = np.ascontiguousarray(np.repeat(np.asarray(vm, dtype=np.float64), pn))
    D = np.ascontiguousarray(np.repeat(np.asarray(stif, dtype=np.int64).reshape(n, 5), pn, axis=0))
    tab = np.ascontiguousarray(tab, dtype=np.float64)
    pt, ps, pa, pb, pc, pd, ptab = (a.ctypes.data for a in (ttn, nsts, A, B, C, D, tab))
    ncol = tab.shape[1]
    out = np.empty(n)
    iz, ix, nnz, nnx = ([int(v) for v in a] for a in (iz, ix, nnz, nnx))
    dnx = [float(v) for v in dnx]
    son = [bool(v) for v in stif_on]
    for k in range(n):
        o = k * pn
        sp = pd + 40 * o if son[k] else None
        if op == 0:
            out[k] = L.oref_update(pz, px, pt + 8 * o, ps + 4 * o, iz[k], ix[k], dnx[k], nnz[k], nnx[k], pa + 8 * o,
                                   pb + 8 * o, pc + 8 * o, sp, ptab, ncol)
        else:
            assert nnz[k] == pz and nnx[k] == px
            out[k] = L.oref_fouds18(pz, px, pt + 8 * o, ps + 4 * o, iz[k], ix[k], dnx[k], dnx[k], pa + 8 * o, pb + 8 * o,
                                    pc + 8 * o, sp, ptab, ncol)
    return out


def reference(cs, build=None):
    """The oracle's values of a set (build: O.LIB_CR by default), computed once per process."""
    build = O.LIB_CR if build is None else build
    key = (cs.name, build)
    if key not in _refs:
        r = oracle_values(cs.op, build, cs.ttn, cs.nsts, cs.iz, cs.ix, cs.dnx, cs.nnz, cs.nnx, *case_mats(cs), table(cs))
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


# ---- the reference-made neighbourhoods of tests/golden/local_ops.npz as a third input set ------
def golden_sets(g):
    """(update set, fouds18_A() set, their materials and tables) from the golden file `g`."""
    if "g" not in _sets:
        a, f = g["u_args"], g["f_args"]
        nu, nf = len(a), len(f)
        z = np.zeros
        u = CaseSet("golden_update", 0, g["u_ttn"], g["u_nsts"].astype(np.int32), a[:, 0].astype(np.int32),
                    a[:, 1].astype(np.int32), a[:, 2].copy(), a[:, 3].astype(np.int32), a[:, 4].astype(np.int32),
                    None, z(nu, np.int64), z(nu, np.int64), z(nu, np.int64))
        s = CaseSet("golden_fouds18", 1, g["f_ttn"], g["f_nsts"].astype(np.int32), f[:, 0].astype(np.int32),
                    f[:, 1].astype(np.int32), f[:, 2].copy(), np.full(nf, 7, np.int32), np.full(nf, 7, np.int32),
                    None, z(nf, np.int64), z(nf, np.int64), z(nf, np.int64))
        _sets["g"] = (u, s)
    return _sets["g"]


def golden_mats(g, cs):
    p = "u_" if cs.op == 0 else "f_"
    m = g[p + "mat"]
    n = len(m)
    return m[:, 0].copy(), m[:, 1].astype(np.int64), m[:, 2].copy(), np.ones(n, dtype=bool), g[p + "stif"].astype(np.int64)


def golden_reference(g, cs, build=None):
    build = O.LIB_CR if build is None else build
    key = (cs.name, build)
    if key not in _refs:
        r = oracle_values(cs.op, build, cs.ttn, cs.nsts, cs.iz, cs.ix, cs.dnx, cs.nnz, cs.nnx, *golden_mats(g, cs),
                          g["tab_p" if cs.op == 0 else "tab_g"])
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


# ---- the resident models of the PRE_ONLY forms --------------------------------------------------
def resident_models():
    """(name, (veln, velpn, vm, stif), dnx) of test_band_fouds18_path_vs_oracle: the weld (table
    columns) and C3 at 512 (per-cell stiffness, velpn 0 in every grain)."""
    import workloads as W

    return (("weld", W.weld_model(), 2e-4), ("c3", W.c3_model(512), 1e-3))


def resident_cells(name, shape, n):
    rng = np.random.default_rng({"weld": 41, "c3": 42}[name])
    return rng.integers(0, shape[0], n).astype(np.int32), rng.integers(0, shape[1], n).astype(np.int32)


def resident_reference(name, model, quant, cs, mz, mx, tab, build=None):
    """oref_fouds18 (the correctly rounded build by default) on the material of model cell (mz, mx)
    under the view `quant` (1: orientation truncated to int32, vel_map rounded to float32)."""
    build = O.LIB_CR if build is None else build
    key = (cs.name, name, quant, build)
    if key not in _refs:
        veln, velpn, vm, sd = model
        a, b = veln[mz, mx], vm[mz, mx]
        if quant:
            a, b = np.trunc(a).astype(np.int32).astype(np.float64), b.astype(np.float32).astype(np.float64)
        n = len(mz)
        son = np.full(n, sd is not None)
        st = sd[mz, mx] if sd is not None else np.zeros((n, 5), dtype=np.int64)
        r = oracle_values(1, build, cs.ttn, cs.nsts, cs.iz, cs.ix, cs.dnx, cs.nnz, cs.nnx, a, velpn[mz, mx], b, son, st,
                          tab)
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]
