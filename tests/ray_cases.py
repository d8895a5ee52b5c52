"""The small-shape case matrix of the ray tracer (csrc/rays.hip find_ray_kernel / tbp_wave, utils.hip
tbp_kernel) against the CPU oracle (oracle/alifmm_oracle.c find_ray_impl / tbp_impl), shared by
tests/test_oracle.py (the oracle's side: test_ray_case_matrix_preconditions) and
tests/test_gpu_rays_small.py (the device's side, on the same uploaded fields).

Everything is deterministic: seeded generators, coordinates given on the fine grid (x, z) as the
library takes them (fine = subgrid * coarse).  The matrix is a set of axes around a default, not
their product.  Grids (nz x nx, coarse nodes):
  * segment cases: 21 x 300 (SEG_H, column stripes) and 300 x 21 (SEG_V, the same layout transposed);
    subgrid 3 fields are 61 x 898 and 898 x 61;
  * walk cases: 41 x 57 and 57 x 41 (grain, mixed, iso), 2 x 57 and 41 x 3 (grain), 61 x 61 (iso:
    the capacity ring and the position / batch list); subgrid 11 fields of 41 x 57 are 441 x 617.

Segment cases test time_between_points one segment at a time through the ray kernel: on a "pit"
field (0.0 at the node the source rounds to, 1.0 elsewhere) the walk stops at its first step (the
field increases: the early exit), or is not entered (the receiver within 1.6 subgrid nodes), or its
first axis plane leaves the grid; in every case the ray is [source, receiver] and its time is that
one segment's, evaluated by tbp_wave in the kernel's ray_time loop.  Segments that share a pit share
a field.  Walk cases are whole rays on uploaded fields.
"""
import collections

import numpy as np

import band_cases as BC
import oracle as O
import workloads as W

DNX = 1e-3
TABLE = BC.TABLE

Model = collections.namedtuple("Model", "name nz nx veln velpn vm sd table ids")

# ---- the models ----
SEG_H = (21, 300)
SEG_V = (300, 21)
# records by name -> (distinct records, LDS tables in the ray kernel).  af_launch_rays (rays.hip)
# stages the tables in LDS when nmat <= 256 and stiffness rows <= 64 and 361 * ncol <= 722:
#   m257 fails the first (nmat 257), stif65 the second (65 rows, nmat 65), vt3 the third (ncol 3:
#   1083 doubles, nmat 6) -> the LDSMAT = false instantiations.
SEG_MODELS = {"iso": (1, True), "stripes": (6, True), "mixed": (None, True), "m256": (256, True),
              "m257": (257, False), "stif65": (65, False), "vt3": (6, False)}
WALK_MODELS = ("iso", "grain", "mixed")


def stripe_index():
    """Palette index of each of the 300 stripes (columns of SEG_H, rows of SEG_V) of the `stripes`
    model: one-column stripes 12..18 between long ones, a lone boundary at 276 (256 nodes from 20),
    an A B A at 281 | 282, 283 | 284."""
    s = np.zeros(300, dtype=np.int64)
    s[10:12] = 1
    s[12], s[13], s[14], s[15], s[16], s[17], s[18] = 2, 3, 4, 5, 1, 2, 3
    s[276:300] = 1
    s[282:284] = 0
    return s


def _table3():
    """A 3-column velocity table: angle, ones, and a smooth angle-dependent column."""
    t = np.ones((361, 3))
    t[:, 0] = np.arange(361)
    t[:, 2] = 1.0 + 0.125 * np.cos(np.deg2rad(2.0 * np.arange(361)))
    return t


TABLE3 = _table3()
_models = {}


def _stripe_palette(name):
    """(index per stripe, veln, velpn, vm, stiffness rows or None, table) of a stripe model."""
    k300 = np.arange(300)
    row = W.STIF_ROW
    if name == "iso":
        return np.zeros(300, dtype=np.int64), np.zeros(1), np.ones(1, np.int64), np.full(1, 5790.0), None, TABLE
    if name == "stripes":
        return (stripe_index(), np.array([0.0, 35.0, 70.5, 110.0, 150.0, 20.0]),
                np.array([0, 0, 1, 0, 0, 0], np.int64), np.array([1.0, 1.0, 5790.0, 1.125, 1.0, 1.0]),
                np.tile(row, (6, 1)), TABLE)
    if name in ("m256", "m257"):
        n = int(name[1:])
        k = np.arange(n)
        velpn = (k % 5 == 3).astype(np.int64)
        return (k300 % n, 0.7 * k, velpn, np.where(velpn == 1, 5790.0, 1.0), np.tile(row, (n, 1)), TABLE)
    if name == "stif65":
        k = np.arange(65)
        sd = np.tile(row, (65, 1))
        sd[:, 0] += 1000 * k
        sd[:, 2] += 500 * k
        return k300 % 65, 2.5 * k, np.zeros(65, np.int64), np.ones(65), sd, TABLE
    if name == "vt3":
        return (stripe_index(), np.array([0.0, 35.0, 70.5, 110.0, 150.0, 20.0]),
                np.array([0, 1, 2, 0, 2, 1], np.int64), np.array([1.0, 5790.0, 5000.0, 1.125, 6100.0, 5790.0]),
                np.tile(row, (6, 1)), TABLE3)
    raise KeyError(name)


def model(name, nz, nx):
    """A named model on an nz x nx grid; cached, never modified.  `ids`: a per-cell record number
    (equal numbers: equal records), what the run classes of a segment are counted with."""
    key = (name, nz, nx)
    if key in _models:
        return _models[key]
    if name in ("grain", "mixed") or (name == "iso" and (nz, nx) not in (SEG_H, SEG_V)):
        veln, velpn, vm, sd = BC.model_arrays(name, nz, nx)
        cols = np.stack([veln.ravel(), velpn.ravel().astype(np.float64), vm.ravel()], -1)
        ids = np.unique(cols, axis=0, return_inverse=True)[1].reshape(nz, nx)
        m = Model(name, nz, nx, veln, velpn, vm, sd, TABLE, ids)
    else:
        assert (nz, nx) in (SEG_H, SEG_V), (name, nz, nx)
        idx, veln, velpn, vm, rows, table = _stripe_palette(name)
        ids = np.tile(idx, (21, 1))
        if (nz, nx) == SEG_V:
            ids = np.ascontiguousarray(ids.T)
        sd = None if rows is None else np.ascontiguousarray(rows[ids])
        m = Model(name, nz, nx, np.ascontiguousarray(veln[ids]), np.ascontiguousarray(velpn[ids]),
                  np.ascontiguousarray(vm[ids]), sd, table, ids)
    for a in m:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _models[key] = m
    return m


def set_model(ctx, m):
    ctx.set_model(m.veln, m.velpn, m.vm, m.sd, m.table, m.table, DNX)


def record_count(m):
    return len(np.unique(m.ids))


def stiffness_rows(m):
    return 0 if m.sd is None else len(np.unique(m.sd.reshape(-1, 5), axis=0))


# ---- segments ----
# fine-grid coordinates; pieces / runs: the classes the name states (None: not stated), runs on the
# `stripes` model
Seg = collections.namedtuple("Seg", "name x1 y1 x2 y2 pieces runs")
NODE_L = (1, 2, 7, 8, 11, 12, 254, 255, 256)


def walk_cells(x1, x2, y1, y2, sg, limit=None):
    """The (row, column) of every piece of time_between_points' walk over a segment, in order: the
    geometry of tbp_impl (oracle/alifmm_oracle.c) restated, to count a case's pieces and runs.
    None past `limit` pieces: a horizontal segment at z = k + 0.5, k odd, starts with next_y == end_y,
    the strict '<' never sets fin_y and the walk does not end (the capacity ray holds such segments,
    which is why a ray cut short is not timed)."""
    x1, x2, y1, y2 = x1 / float(sg), x2 / float(sg), y1 / float(sg), y2 / float(sg)
    mm = cc = 0.0
    if x2 != x1:
        mm = (y2 - y1) / (x2 - x1)
        cc = y1 - mm * x1
    fin_x = fin_y = False
    dir_x = 1 if x1 < x2 else -1
    dir_y = 1 if y1 < y2 else -1
    next_x = round(x1) + dir_x * 0.5
    next_y = round(y1) + dir_y * 0.5
    px, py = x1, y1
    cells = []
    while not (fin_x and fin_y):
        if ((next_x > x2 and dir_x == 1) or (next_x < x2 and dir_x == -1)) and not fin_x:
            fin_x, next_x = True, x2
        if ((next_y > y2 and dir_y == 1) or (next_y < y2 and dir_y == -1)) and not fin_y:
            fin_y, next_y = True, y2
        if x2 == x1:
            nxv, nyv = x1, next_y
            next_y += dir_y
        else:
            yv = mm * next_x + cc
            if mm != 0:
                xv = (next_y - cc) / mm
                d1 = (x1 - next_x) * (x1 - next_x) + (y1 - yv) * (y1 - yv)
                d2 = (x1 - xv) * (x1 - xv) + (y1 - next_y) * (y1 - next_y)
                if d1 < d2:
                    nxv, nyv = next_x, yv
                    next_x += dir_x
                else:
                    nxv, nyv = xv, next_y
                    next_y += dir_y
            else:
                nxv, nyv = next_x, yv
                next_x += dir_x
        cells.append((round((py + nyv) / 2), round((px + nxv) / 2)))
        px, py = nxv, nyv
        if limit is not None and len(cells) > limit:
            return None
    return cells


def seg_classes(m, s, sg):
    """(pieces, runs, first piece of each run after the first, record of each run) of a segment."""
    cells = walk_cells(s.x1, s.x2, s.y1, s.y2, sg)
    ids = [int(m.ids[z, x]) for z, x in cells]
    starts = [k for k in range(1, len(ids)) if ids[k] != ids[k - 1]]
    return len(ids), len(starts) + 1, starts, [ids[0]] + [ids[k] for k in starts]


def _both(name, a, b, pieces=None, runs=None):
    """A segment a -> b (coarse nodes) and its reverse."""
    return [(name, a, b, pieces, runs), (name + "_rev", b, a, pieces, runs)]


def _node_segments_h():
    """The designed segments of SEG_H in coarse nodes (x, z): name, from, to, pieces, runs."""
    out = []
    z = 10
    # from column 2 across the one-column stripes: a horizontal node-to-node segment of L nodes has
    # L + 1 pieces, piece k in column 2 + k
    runs2 = {1: 1, 2: 1, 7: 1, 8: 2, 11: 4, 12: 5, 254: 10, 255: 10, 256: 10}
    for L in NODE_L:
        out += _both("h2_L%d" % L, (2, z), (2 + L, z), L + 1, runs2[L])
    # from column 20: one run, the last boundary at piece 256 (piece indices past 255 force `over`)
    for L, r in ((254, 1), (255, 1), (256, 2)):
        out += _both("h20_L%d" % L, (20, z), (20 + L, z), L + 1, r)
    out += _both("h3_L8_change7", (3, z), (11, z), 9, 2)
    out += _both("h265_L11_change11", (265, z), (276, z), 12, 2)
    out += _both("h265_L12_change11", (265, z), (277, z), 13, 2)
    out += _both("h264_L12_change12", (264, z), (276, z), 13, 2)
    out += _both("h279_L8_aba", (279, z), (287, z), 9, 3)
    out += _both("h6_L12_runs9", (6, z), (18, z), 13, 9)
    out += _both("h9_L4_runs4", (9, z), (13, z), 5, 4)
    out += _both("h9_L5_runs5", (9, z), (14, z), 6, 5)
    # vertical, inside one stripe (column 13)
    for L in (1, 2, 7, 8, 11, 12):
        out += _both("v13_L%d" % L, (13, 2), (13, 2 + L), L + 1, 1)
    # exact 45 degree diagonals through nodes, both signs
    out += _both("d_2_2_L12", (2, 2), (14, 14))
    out += _both("d_14_2_L12", (14, 2), (2, 14))
    out += _both("d_8_4_L11", (8, 4), (19, 15))
    out += _both("d_270_18_L7", (270, 18), (277, 11))
    # ending on (and running along) the last row and column, and the first
    out += _both("d_to_corner", (285, 6), (299, 20))
    out += _both("lastrow_L29", (270, 20), (299, 20), 30, 4)
    out += _both("lastcol_L17", (299, 3), (299, 20), 18, 1)
    out += _both("firstrow_L12", (0, 0), (12, 0), 13, 3)
    out += _both("firstcol_L12", (0, 0), (0, 12), 13, 1)
    # zero length
    out.append(("zero_node", (13, 10), (13, 10), 1, 1))
    return out


def _oblique(sg, shape, pits, n_each, seed):
    """Seeded oblique segments with fractional endpoints (multiples of 1/64 of a fine node): sources
    within 0.4 of a pit node (off exact .5, towards the grid's inside on an edge), receivers anywhere
    in the grid, the even ones within 15 coarse nodes."""
    nz, nx = shape
    fx, fz = sg * (nx - 1), sg * (nz - 1)
    rng = np.random.default_rng(seed)
    out = []
    for p, (px, pz) in enumerate(pits):
        for k in range(n_each):
            ox, oz = rng.integers(-25, 26, 2) / 64.0
            sx = min(max(sg * px + ox, 0.0), float(fx))
            sz = min(max(sg * pz + oz, 0.0), float(fz))
            if k % 2 == 0:
                rx = min(max(sx + rng.integers(-15 * 64 * sg, 15 * 64 * sg + 1) / 64.0, 0.0), float(fx))
                rz = min(max(sz + rng.integers(-15 * 64 * sg, 15 * 64 * sg + 1) / 64.0, 0.0), float(fz))
            else:
                rx = rng.integers(0, 64 * fx + 1) / 64.0
                rz = rng.integers(0, 64 * fz + 1) / 64.0
            out.append(Seg("obl_p%d_%d" % (p, k), sx, sz, rx, rz, None, None))
    return out


OBLIQUE_PITS_H = ((5, 3), (14, 10), (60, 17), (150, 10), (270, 4), (281, 12), (299, 20), (0, 0))
_segs = {}


def segments(shape, sg):
    """The segment cases of a grid (SEG_H or SEG_V) at a subgrid.  SEG_V holds SEG_H's designed
    segments transposed (its stripes are rows): the vertical node-to-node classes."""
    key = (shape, sg)
    if key in _segs:
        return _segs[key]
    out = []
    for name, a, b, pieces, runs in _node_segments_h():
        if shape == SEG_H:
            out.append(Seg(name, float(sg * a[0]), float(sg * a[1]), float(sg * b[0]), float(sg * b[1]), pieces, runs))
        else:
            out.append(Seg("t_" + name, float(sg * a[1]), float(sg * a[0]), float(sg * b[1]), float(sg * b[0]),
                           pieces, runs))
    if shape == SEG_H:
        out.append(Seg("zero_frac", sg * 13 + 0.25, sg * 10 + 0.125, sg * 13 + 0.25, sg * 10 + 0.125, 1, 1))
        out += _oblique(sg, shape, OBLIQUE_PITS_H, 25, 100 + sg)
    else:
        out += _oblique(sg, shape, [(z, x) for x, z in OBLIQUE_PITS_H[:4]], 6, 200 + sg)
    _segs[key] = out
    return out


def ray_segments(shape, sg):
    """(numbers, segments) of the segment cases that go through the ray kernel.  Not the exact
    diagonals at subgrid 1: the first search plane of a diagonal step lies 0.7 nodes from the source,
    its minimum on a uniform field falls half way between two nodes and rounds (half-even) back onto
    the pit, so the walk goes on.  Those rays are the walk batch DIAG_TIE_BATCH (the kernel reads
    rec_TTF off the search plane there); time_between_points takes every segment."""
    segs = segments(shape, sg)
    keep = [k for k, s in enumerate(segs) if not (sg == 1 and s.name.lstrip("t_").startswith("d_"))]
    return np.array(keep), [segs[k] for k in keep]


def pit_of(s):
    """The fine node (x, z) the segment's source rounds to (Python round: half-even, as pyround)."""
    return round(s.x1), round(s.y1)


def pits(segs):
    """The distinct pits of a segment list, in order of first use, and each segment's pit number."""
    order, idx = [], []
    for s in segs:
        p = pit_of(s)
        if p not in order:
            order.append(p)
        idx.append(order.index(p))
    return order, np.array(idx, dtype=np.int32)


def pit_field(shape, sg, pit):
    nz, nx = shape
    f = np.ones((sg * (nz - 1) + 1, sg * (nx - 1) + 1))
    f[pit[1], pit[0]] = 0.0
    return f


# the (model, grid) pairs the segment cases run on
SEGMENT_RUNS = [(m, SEG_H) for m in SEG_MODELS] + [("stripes", SEG_V), ("m257", SEG_V)]
SEG_SUBGRIDS = (1, 3)

# ---- walks ----
# a field: kind "travel" (the oracle's field of a source at coarse node p), "dist" (Euclidean
# distance to the fine point p times dnx / sg / 5790: an isotropic field for nothing), "ring"
# (0.0 where |r - 20| <= 2.5 around p, 1.0 elsewhere) or "pit" (0.0 at the fine node p, 1.0 elsewhere)
Field = collections.namedtuple("Field", "kind p")
Batch = collections.namedtuple("Batch", "name model nz nx sg fields rays")  # rays: (field number, source, receiver)
_fields = {}


def field_array(b, k):
    """Field k of a batch, (fnz, fnx) float64; cached, never modified."""
    f = b.fields[k]
    key = (b.model if f.kind == "travel" else None, b.nz, b.nx, b.sg, f)
    if key in _fields:
        return _fields[key]
    m = model(b.model, b.nz, b.nx)
    fz, fx = b.sg * (b.nz - 1) + 1, b.sg * (b.nx - 1) + 1
    if f.kind == "pit":
        a = pit_field((b.nz, b.nx), b.sg, f.p)
    elif f.kind == "travel":
        x, z = DNX * f.p[0], DNX * f.p[1]
        if b.sg == 1:
            a = O.travel(x, z, m.veln, m.velpn, m.vm, m.sd, m.table, m.table, dnx=DNX)
        else:
            a = O.travel_finer_grid(x, z, m.veln, m.velpn, m.vm, m.sd, b.sg, m.table, m.table, dnx=DNX)
    elif f.kind == "dist":
        zz, xx = np.mgrid[0:fz, 0:fx]
        a = np.hypot(xx - f.p[0], zz - f.p[1]) * (DNX / b.sg / 5790.0)
    elif f.kind == "ring":
        zz, xx = np.mgrid[0:fz, 0:fx]
        a = np.where(np.abs(np.hypot(xx - f.p[0], zz - f.p[1]) - 20.0) <= 2.5, 0.0, 1.0)
    else:
        raise KeyError(f.kind)
    assert a.shape == (fz, fx)
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    _fields[key] = a
    return a


def walk_sources(nz, nx, rec, seed, n_seeded=20):
    """Source nodes (x, z) of a grid for a receiver node: the corners, the edge midpoints, the
    receiver itself and nodes next to it (inside 1.6 nodes: the walk is not entered; just outside),
    and seeded interior nodes."""
    cx, cz = nx - 1, nz - 1
    s = [(0, 0), (cx, 0), (0, cz), (cx, cz), (nx // 2, 0), (nx // 2, cz), (0, nz // 2), (cx, nz // 2),
         rec, (rec[0] + 1, rec[1]), (rec[0] + 1, rec[1] + 1), (rec[0] - 2, rec[1]), (rec[0], rec[1] + 2)]
    rng = np.random.default_rng(seed)
    if nz > 2 and nx > 2:
        s += [(int(rng.integers(1, cx)), int(rng.integers(1, cz))) for _ in range(n_seeded)]
    else:
        s += [(int(rng.integers(0, nx)), int(rng.integers(0, nz))) for _ in range(n_seeded)]
    return [(min(max(x, 0), cx), min(max(z, 0), cz)) for x, z in s]


def _field_batch(name, mname, shape, sg, kind, recs, seed):
    """One field per receiver node and walk_sources' rays to each."""
    nz, nx = shape
    fields, rays = [], []
    for k, r in enumerate(recs):
        fields.append(Field(kind, r if kind == "travel" else (sg * r[0], sg * r[1])))
        for s in walk_sources(nz, nx, r, seed + k):
            rays.append((k, (float(sg * s[0]), float(sg * s[1])), (float(sg * r[0]), float(sg * r[1]))))
    return Batch(name, mname, nz, nx, sg, tuple(fields), tuple(rays))


def _receivers(nz, nx):
    """An interior receiver and one on the top edge."""
    return [(nx // 3 + 1, nz // 2 + 2), (nx // 2 + 3, 0)]


# oracle fields on the grain and mixed models at subgrids 1 and 3 (16-lane and 32-lane groups)
TRAVEL_BATCHES = [_field_batch("%s_%dx%d_sg%d" % (m, nz, nx, sg), m, (nz, nx), sg, "travel", _receivers(nz, nx), 7)
                  for m in ("grain", "mixed") for nz, nx in ((41, 57), (57, 41)) for sg in (1, 3)]
# synthetic isotropic fields at subgrids 5, 9 (64-lane groups) and 11 (69 candidates: two rounds)
DIST_BATCHES = [_field_batch("iso_41x57_sg%d" % sg, "iso", (41, 57), sg, "dist", _receivers(41, 57), 11)
                for sg in (5, 9, 11)]
# grids the search planes hang over: 2 rows, 3 columns (subgrid 1, grain)
THIN_BATCHES = [_field_batch("grain_2x57_sg1", "grain", (2, 57), 1, "travel", [(20, 1), (40, 0)], 13),
                _field_batch("grain_41x3_sg1", "grain", (41, 3), 1, "travel", [(1, 15), (2, 30)], 17)]
WALK_BATCHES = TRAVEL_BATCHES + DIST_BATCHES + THIN_BATCHES

# ---- one case per exit of the walk (41 x 57 isotropic model, every subgrid) ----
EXIT_SUBGRIDS = (1, 3, 5, 9, 11)
# name -> (rc class, early, points) the oracle returns; "n" a complete ray.  The empty plane needs
# diagonal planes narrower than one node: at subgrid 1 that ray completes.
EXIT_EXPECT = {"early": ("n", 1, 72), "leaves_grid": ("n", 0, 48), "empty_plane": (-4, 0, None)}


def exit_batch(sg):
    """The early exit (flag 1), an axis plane leaving the grid (no flag), the empty plane (flag 4,
    subgrid >= 3) and walks that are not entered (the receiver itself, a source 1.5 subgrid nodes
    from it)."""
    nz, nx = 41, 57
    fx = sg * (nx - 1) + 1
    f = (Field("dist", (40 * sg, 5 * sg)), Field("dist", (fx - 1, 20 * sg)), Field("dist", (0, 0)))
    s = float(sg)
    rays = ((0, (3 * s, 38 * s), (52 * s, 2 * s)),
            (1, (10 * s, 20 * s), (30 * s, 2 * s)),
            (2, (26 * s, 26 * s), (50 * s, 5 * s)),
            (0, (52 * s, 2 * s), (52 * s, 2 * s)),
            (0, (52 * s - 1.5 * s, 2 * s), (52 * s, 2 * s)),
            (1, (30 * s + 1.0, 2 * s + 1.25 * s), (30 * s, 2 * s)),
            (1, (30 * s + 0.96 * s, 2 * s + 1.28 * s), (30 * s, 2 * s)))
    return Batch("exits_sg%d" % sg, "iso", nz, nx, sg, f, rays)


# (near_1.6: 1.6008 nodes at subgrid 1, inside 1.6 sg above; on_1.6: 0.96^2 + 1.28^2 = 1.6^2, the
# loop condition's own rounding decides)
EXIT_NAMES = ("early", "leaves_grid", "empty_plane", "not_entered_same", "not_entered_1.5", "near_1.6", "on_1.6")
EXIT_BATCHES = [exit_batch(sg) for sg in EXIT_SUBGRIDS]

# ---- the point capacity (flag 2) and the position / batch list: 61 x 61 isotropic, subgrid 1 ----
CAP_POINTS = 5 * (61 + 61)  # 610: the oracle returns -3 having written 609 points


def mix_batch():
    """One list holding 2-point rays, the capacity ray (orbiting the ring: 610 points), an early
    exit and ordinary rays, on three fields of one 61 x 61 model: what the position and batch
    independence tests permute."""
    c = 30
    f = (Field("ring", (c, c)), Field("dist", (40, 5)), Field("dist", (20, 31)))
    rays = [(0, (c + 20.0, float(c)), (c + 23.0, 58.0)),      # capacity
            (1, (3.0, 50.0), (56.0, 2.0)),                     # early exit (the field's minimum is elsewhere)
            (2, (20.0, 31.0), (20.0, 31.0)),                   # 2 points: the receiver itself
            (2, (21.0, 32.0), (20.0, 31.0)),                   # 2 points: inside 1.6 nodes
            (2, (58.0, 3.0), (20.0, 31.0)), (2, (0.0, 0.0), (20.0, 31.0)), (2, (60.0, 60.0), (20.0, 31.0)),
            (2, (22.0, 31.0), (20.0, 31.0)), (1, (10.0, 55.0), (40.0, 5.0)), (1, (41.0, 7.0), (40.0, 5.0)),
            (2, (3.25, 40.5625), (20.0, 31.0)), (1, (59.0, 30.0), (40.0, 5.0)), (2, (30.0, 0.0), (20.0, 31.0)),
            (1, (0.0, 5.0), (40.0, 5.0)), (2, (20.0, 60.0), (20.0, 31.0)), (1, (40.0, 60.0), (40.0, 5.0)),
            (2, (45.0, 45.0), (20.0, 31.0))]
    return Batch("mix_61x61_sg1", "iso", 61, 61, 1, f, tuple(rays))


MIX_BATCH = mix_batch()
CAP_RAY = 0  # MIX_BATCH.rays[0]


# the exact diagonals at subgrid 1 on their pit fields (ray_segments): 3- and 4-point rays
def _diag_tie_batch():
    segs = [s for s in segments(SEG_H, 1) if s.name.startswith("d_")]
    order, idx = pits(segs)
    return Batch("diag_ties_21x300_sg1", "iso", 21, 300, 1, tuple(Field("pit", p) for p in order),
                 tuple((int(k), (s.x1, s.y1), (s.x2, s.y2)) for k, s in zip(idx, segs)))


DIAG_TIE_BATCH = _diag_tie_batch()


# ---- the oracle's side ----
def oracle_model(m):
    return O.model(m.table, m.veln, m.velpn, m.vm, m.sd)


Ref = collections.namedtuple("Ref", "rc early x y t walked")
_refs = {}


def batch_reference(b, lib_path):
    """The oracle's result (Ref) of every ray of a batch from one build of the restatement
    (O.LIB_GLIBC, O.LIB_CR); cached, shared by the tests of a session."""
    key = (b.name, lib_path)
    if key not in _refs:
        L = O.open_lib(lib_path)
        om = oracle_model(model(b.model, b.nz, b.nx))
        _refs[key] = [Ref(*O.find_ray_walked(DNX, om, s, r, field_array(b, k), None, None, None, None, b.sg, lib=L))
                      for k, s, r in b.rays]
    return _refs[key]


def segment_batch(mname, shape, sg):
    """The segment cases of a model as a batch: one pit field per distinct pit."""
    segs = ray_segments(shape, sg)[1]
    order, idx = pits(segs)
    return Batch("seg_%s_%dx%d_sg%d" % (mname, shape[0], shape[1], sg), mname, shape[0], shape[1], sg,
                 tuple(Field("pit", p) for p in order),
                 tuple((int(k), (s.x1, s.y1), (s.x2, s.y2)) for k, s in zip(idx, segs)))


def segment_times(mname, shape, sg, lib_path):
    """time_between_points of every segment case of a model from one build of the restatement."""
    key = ("tbp", mname, shape, sg, lib_path)
    if key not in _refs:
        L = O.open_lib(lib_path)
        om = oracle_model(model(mname, *shape))
        _refs[key] = np.array([O.time_between_points(s.x1, s.x2, s.y1, s.y2, DNX, sg, om, None, None, None, None,
                                                     lib=L) for s in segments(shape, sg)])
    return _refs[key]
