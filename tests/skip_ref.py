"""The contract of alifmm_skip_pick / alifmm_skip_rays (include/alifmm.h) restated in numpy: the pick
of the specular node and the join of the two legs, the case matrix the CPU and GPU tests share, its
oracle composition (pick on oracle fields, two oracle rays, joined), and the input file of the
stand-alone host run of the kernels' per-element code (tests/skip_sim.cpp).  Test infrastructure only.
"""
import collections

import numpy as np

import oracle as O
import ray_cases as RC

NO_HIT = 8  # flag of a pair without a candidate


def pick(fields, slot_a, slot_b, w_iz, w_ix):
    """(pick_time float64 [npairs], hit int32 [npairs]) of pairs of `fields` (nf, fnz, fnx): per pair
    the lowest node number among the least finite sums fields[a] + fields[b] at the nodes; -1 and
    +inf with no finite sum."""
    fields = np.asarray(fields, dtype=np.float64)
    W = fields[:, np.asarray(w_iz), np.asarray(w_ix)]
    return pick_rows(W, slot_a, slot_b)


def pick_rows(W, row_a, row_b):
    """pick() on gathered values W (nf, nw)."""
    W = np.asarray(W, dtype=np.float64)
    n = len(row_a)
    pt, hit = np.full(n, np.inf), np.full(n, -1, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for k in range(n):
            s = W[row_a[k]] + W[row_b[k]]
            fin = np.isfinite(s)
            if fin.any():
                q = int(np.argmin(np.where(fin, s, np.inf)))  # the first of the least
                hit[k], pt[k] = q, s[q]
    return pt, hit


def join(leg_a, leg_b):
    """The joined ray of two legs ((n, 2) points, both starting at the hit node): leg A reversed, then
    leg B from its second point on."""
    leg_a, leg_b = np.asarray(leg_a).reshape(-1, 2), np.asarray(leg_b).reshape(-1, 2)
    return np.concatenate([leg_a[::-1], leg_b[1:]])


def compose(hit, legs):
    """Joined request from per-pair hits and leg results: legs[k] = ((tA, lenA, flagsA, ptsA), (tB, ...))
    or None for a pair without a hit.  Returns (times, lens, flags, list of point arrays)."""
    n = len(hit)
    t, ln, fl, pts = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), []
    for k in range(n):
        if hit[k] < 0:
            fl[k] = NO_HIT
            pts.append(np.zeros((0, 2)))
            continue
        (ta, la, fa, pa), (tb, lb, fb, pb) = legs[k]
        assert la == len(pa) and lb == len(pb)
        p = join(pa, pb)
        ln[k], fl[k] = len(p), fa | fb
        t[k] = 0.0 if fl[k] & 6 else ta + tb
        pts.append(p)
    return t, ln, fl, pts


# ---- the case matrix: five elements on the top row, the reflector on the last fine row, every pair a <= b ----
Case = collections.namedtuple("Case", "name model nz nx sg")
CASES = [Case("%s_%dx%d_sg%d" % (m, nz, nx, sg), m, nz, nx, sg)
         for m, nz, nx in (("iso", 41, 61), ("grain", 41, 57), ("mixed", 41, 57), ("grain", 57, 41)) for sg in (1, 3)]
NELEM = 5


def elements(c):
    """The elements' coarse x nodes (top row)."""
    return [int(round(f * (c.nx - 1))) for f in (0.1, 0.3, 0.5, 0.7, 0.9)]


def pairs(n=NELEM):
    return [(a, b) for a in range(n) for b in range(a, n)]


def batch(c):
    """The case's fields as a ray_cases.Batch (cached oracle fields of the elements)."""
    return RC.Batch("skip_" + c.name, c.model, c.nz, c.nx, c.sg, tuple(RC.Field("travel", (x, 0)) for x in elements(c)), ())


def fields(c):
    b = batch(c)
    return np.stack([RC.field_array(b, k) for k in range(NELEM)])


def back_wall(c):
    """(w_iz, w_ix) of the last fine row."""
    fz, fx = c.sg * (c.nz - 1) + 1, c.sg * (c.nx - 1) + 1
    return np.full(fx, fz - 1, dtype=np.int32), np.arange(fx, dtype=np.int32)


def request(c):
    """(slot_a, slot_b, a_xy, b_xy) of the case's 15 pairs; slots are element numbers."""
    pr = np.array(pairs(), dtype=np.int32)
    ex = np.array(elements(c), dtype=np.float64) * c.sg
    xy = np.stack([ex, np.zeros(NELEM)], axis=1)
    return pr[:, 0].copy(), pr[:, 1].copy(), xy[pr[:, 0]], xy[pr[:, 1]]


Composition = collections.namedtuple("Composition", "pick hit legs times lens flags points")
_comp = {}


def oracle_composition(c, lib_path=None):
    """The pick on the oracle fields and the oracle's two legs per pair, joined: the host composition
    the device's skip_rays is compared with.  legs[k] = two RC.Ref.  Cached."""
    lib_path = O.LIB_CR if lib_path is None else lib_path
    key = (c.name, lib_path)
    if key in _comp:
        return _comp[key]
    L = O.open_lib(lib_path)
    F = fields(c)
    om = RC.oracle_model(RC.model(c.model, c.nz, c.nx))
    sa, sb, a_xy, b_xy = request(c)
    w_iz, w_ix = back_wall(c)
    pt, hit = pick(F, sa, sb, w_iz, w_ix)
    refs, legs = [], []
    for k in range(len(sa)):
        src = (float(w_ix[hit[k]]), float(w_iz[hit[k]]))
        two = [RC.Ref(*O.find_ray_walked(RC.DNX, om, src, tuple(xy[k]), F[s[k]], None, None, None, None, c.sg, lib=L))
               for s, xy in ((sa, a_xy), (sb, b_xy))]
        refs.append(two)
        leg = []
        for r, xy in zip(two, (a_xy, b_xy)):
            p = np.stack([r.x, r.y], axis=1)
            if r.rc < 0:  # cut short: the walked points, then the receiver, as the device holds them
                p = np.concatenate([p, [xy[k]]])
            leg.append((r.t, len(p), {-3: 2, -4: 4}.get(r.rc, r.early), p))
        legs.append(tuple(leg))
    t, ln, fl, pts = compose(hit, legs)
    _comp[key] = Composition(pt, hit, refs, t, ln, fl, pts)
    return _comp[key]


def ray_time(c, pts, lib_path=None):
    """ray_time() of a polyline on the case's model: the ordered sum of time_between_points."""
    L = O.open_lib(O.LIB_CR if lib_path is None else lib_path)
    om = RC.oracle_model(RC.model(c.model, c.nz, c.nx))
    t = 0.0
    for i in range(len(pts) - 1):
        t += O.time_between_points(pts[i, 0], pts[i + 1, 0], pts[i, 1], pts[i + 1, 1], RC.DNX, c.sg, om, None, None, None,
                                   None, lib=L)
    return t


# ---- the end-to-end case: iso 41 x 61, six elements on the top row, the back wall on the last row ----
E2E = Case("e2e_iso_41x61_sg1", "iso", 41, 61, 1)
E2E_ELEMENTS = (5, 15, 25, 35, 45, 55)
E2E_BLOCK = (slice(14, 27), slice(22, 39))  # the cells whose vel_map the true model raises by 2 %
# One tomography_step(param="vel_map") from the background with this damping and smoothing lowers
# |measured - times| on the CPU chain (test_skip_ref.py::test_tomography_step_on_the_cpu_chain, which
# prints the ratio).  A Jacobian entry is -time_c / vel_map ~ 1.7e-7 s / 5790 = 3e-11; the values sit
# well below it, so the step is governed by the data.
E2E_DAMP, E2E_SMOOTH = 1e-13, 1e-12


def e2e_models():
    """(background, true) models: RC.Model tuples, the true one with the block's vel_map raised."""
    m = RC.model("iso", 41, 61)
    vm = np.array(m.vm)
    vm[E2E_BLOCK] *= 1.02
    return m, m._replace(vm=vm)


def echo_chain(m, elem_x=E2E_ELEMENTS, lib_path=None):
    """The echo paths of every pair a <= b of elements on the top row of model m (subgrid 1, back wall
    on the last row) by the CPU chain: oracle fields, pick, two oracle rays, join.
    Returns (pairs (n, 2), times, lens, packed points)."""
    L = O.open_lib(O.LIB_CR if lib_path is None else lib_path)
    om = RC.oracle_model(m)
    F = np.stack([O.travel(RC.DNX * x, 0.0, m.veln, m.velpn, m.vm, m.sd, m.table, m.table, dnx=RC.DNX, lib=L)
                  for x in elem_x])
    pr = np.array(pairs(len(elem_x)), dtype=np.int32)
    w_iz, w_ix = np.full(m.nx, m.nz - 1, dtype=np.int32), np.arange(m.nx, dtype=np.int32)
    _, hit = pick(F, pr[:, 0], pr[:, 1], w_iz, w_ix)
    legs = []
    for k, (a, b) in enumerate(pr):
        src = (float(w_ix[hit[k]]), float(w_iz[hit[k]]))
        leg = []
        for e in (a, b):
            r = RC.Ref(*O.find_ray_walked(RC.DNX, om, src, (float(elem_x[e]), 0.0), F[e], None, None, None, None, 1, lib=L))
            assert r.rc > 0
            leg.append((r.t, r.rc, r.early, np.stack([r.x, r.y], axis=1)))
        legs.append(tuple(leg))
    t, ln, fl, pts = compose(hit, legs)
    return pr, t, ln, np.concatenate(pts)


# ---- the stand-alone host run of csrc/skip_pick.h (tests/skip_sim.cpp) ----
def write_sim_input(path, W, row_a, row_b, leg_len, leg_pts, max_pts):
    """int64[8] header (npairs, nw, nf, njoin, max_pts, 0, 0, 0); W float64 [nf][nw]; row_a, row_b int32
    [npairs]; leg_len int32 [2 njoin]; rx, ry float64 [2 njoin][max_pts] (the ray kernel's buffers:
    leg 2 p to a, 2 p + 1 to b; slots past a leg's length hold NaN)."""
    W = np.ascontiguousarray(W, dtype=np.float64)
    nj = len(leg_len) // 2
    rx, ry = np.full((2 * nj, max_pts), np.nan), np.full((2 * nj, max_pts), np.nan)
    for g, p in enumerate(leg_pts):
        rx[g, :len(p)], ry[g, :len(p)] = p[:, 0], p[:, 1]
    with open(path, "wb") as f:
        np.array([len(row_a), W.shape[1], W.shape[0], nj, max_pts, 0, 0, 0], dtype=np.int64).tofile(f)
        W.tofile(f)
        np.ascontiguousarray(row_a, dtype=np.int32).tofile(f)
        np.ascontiguousarray(row_b, dtype=np.int32).tofile(f)
        np.ascontiguousarray(leg_len, dtype=np.int32).tofile(f)
        rx.tofile(f)
        ry.tofile(f)


def read_sim_output(path, npairs, njoin):
    """(pick_time, hit, joined lens, packed points) as skip_sim wrote them."""
    with open(path, "rb") as f:
        pt = np.fromfile(f, dtype=np.float64, count=npairs)
        hit = np.fromfile(f, dtype=np.int32, count=npairs)
        ln = np.fromfile(f, dtype=np.int32, count=njoin)
        pts = np.fromfile(f, dtype=np.float64).reshape(-1, 2)
    return pt, hit, ln, pts
