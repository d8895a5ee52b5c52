"""The contract of alifmm_ray_sens (include/alifmm.h) restated in Python: the reference the device
kernels (csrc/ray_sens.hip) and the host run of their per-segment code (tests/sens_sim.cpp) are
tested against.  Test infrastructure only.

Geometry: time_between_points()'s walk as ray_cases.walk_cells restates it, with each piece's
length, the piece bound B and the validity rules.  Slownesses: Christoffel cells through
oref_group_vel of a build of the oracle (O.open_lib(O.LIB_CR): the device's correctly rounded
trigonometry), table cells in plain Python floats; the segment's angle through the same build's
arctangent where it exports one.
"""
import ctypes
import math

import numpy as np

import oracle as O

H = 2.0 ** -10       # the centred difference's step [degree]
INV_2H = 512.0
RAD2DEG = 180.0 / math.pi


class Model:
    """A model (ray_cases.Model or anything with veln, velpn, vm, sd, table) with one build of the
    oracle for the Christoffel group velocity and the arctangent."""

    def __init__(self, m, lib_path=None, veln=None):
        self.m = m
        self.veln = np.asarray(m.veln if veln is None else veln, dtype=np.float64)
        self.nz, self.nx = self.veln.shape
        self.velpn = np.asarray(m.velpn)
        self.vm = np.asarray(m.vm, dtype=np.float64)
        self.sd = None if m.sd is None else np.asarray(m.sd)
        self.table = np.asarray(m.table, dtype=np.float64)
        self.L = O.open_lib(O.LIB_CR if lib_path is None else lib_path)
        self.atan = math.atan
        if hasattr(self.L, "oref_cr_atan"):
            f = self.L.oref_cr_atan
            f.restype = ctypes.c_double
            f.argtypes = [ctypes.c_double]
            self.atan = f
        self._cache = {}

    def christoffel(self, z, x):
        return int(self.velpn[z, x]) == 0 and self.sd is not None

    def velocity(self, z, x, eff):
        """group_vel_cell of cell (z, x) at effective angle eff."""
        p = int(self.velpn[z, x])
        vm = float(self.vm[z, x])
        if p != 0 or self.sd is None:
            a1 = int(math.floor(eff))
            a2 = (a1 + 1) % 180
            rem = eff - float(a1)
            return vm * ((1 - rem) * float(self.table[a1, p]) + rem * float(self.table[a2, p]))
        s = self.sd[z, x]
        return self.L.oref_group_vel(eff, int(s[0]), int(s[1]), int(s[2]), int(s[3]), int(s[4]), vm)

    def slowness(self, z, x, angle):
        """(s, ds, eff) of cell (z, x) along a segment at `angle` [deg]."""
        rec = (float(self.veln[z, x]), int(self.velpn[z, x]), float(self.vm[z, x]),
               None if self.sd is None else tuple(int(v) for v in self.sd[z, x]), angle)
        if rec not in self._cache:
            eff = (float(self.veln[z, x]) - angle) % 180.0
            s = 1.0 / self.velocity(z, x, eff)
            if self.christoffel(z, x) and snapped(eff):
                ds = 0.0
            else:
                sp = 1.0 / self.velocity(z, x, (eff + H) % 180.0)
                sm = 1.0 / self.velocity(z, x, (eff - H) % 180.0)
                ds = (sp - sm) * INV_2H
            self._cache[rec] = (s, ds, eff)
        return self._cache[rec]


def snapped(eff):
    """The reference's on-axis snap of the Christoffel group velocity."""
    e90 = eff % 90.0
    return e90 < 0.01 or e90 > 90 - 0.01


def axis_distance(eff):
    """Distance [deg] of an effective angle to the nearest axis (0, 90, 180)."""
    e90 = eff % 90.0
    return min(e90, 90.0 - e90)


def piece_bound(x1, x2, y1, y2, sg):
    """B = floor|x2 - x1| + floor|y2 - y1| + 4, coordinates after the division by the subgrid."""
    x1, x2, y1, y2 = x1 / float(sg), x2 / float(sg), y1 / float(sg), y2 / float(sg)
    return math.floor(abs(x2 - x1)) + math.floor(abs(y2 - y1)) + 4


def walk(x1, x2, y1, y2, sg, nz, nx, bound=True):
    """The pieces of a segment, in walk order: a list of (row, column, length in coarse nodes) after
    numba's negative-index wrap, or None when the segment is invalid (a coordinate not finite, a
    cell outside the grid after the wrap, unfinished after B pieces).  bound=False: no piece bound
    (the walk then ends only by leaving the grid); the geometry is ray_cases.walk_cells'."""
    if not all(math.isfinite(v) for v in (x1, x2, y1, y2)):
        return None
    B = piece_bound(x1, x2, y1, y2, sg) if bound else None
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
    out = []
    while not (fin_x and fin_y):
        if B is not None and len(out) >= B:
            return None
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
        mx, my = (px + nxv) / 2, (py + nyv) / 2
        if not (math.isfinite(mx) and math.isfinite(my)):
            return None
        cx, cz = round(mx), round(my)
        if not (-nx <= cx < nx and -nz <= cz < nz):
            return None
        ddx, ddy = px - nxv, py - nyv
        out.append((cz % nz, cx % nx, math.sqrt(ddx * ddx + ddy * ddy)))
        px, py = nxv, nyv
    return out


def segment_angle(M, x1, x2, y1, y2, sg):
    x1, x2, y1, y2 = x1 / float(sg), x2 / float(sg), y1 / float(sg), y2 / float(sg)
    return 0.0 if x1 == x2 else M.atan((y2 - y1) / (x2 - x1)) * RAD2DEG


def segment_entries(M, x1, x2, y1, y2, sg, dnx):
    """The entries of one segment: lists (col, len, time, dth, eff, christoffel), or None when the
    segment is invalid."""
    pieces = walk(x1, x2, y1, y2, sg, M.nz, M.nx)
    if pieces is None:
        return None
    angle = segment_angle(M, x1, x2, y1, y2, sg)
    col, ln, tm, dt, ef, ch = [], [], [], [], [], []
    for z, x, d in pieces:
        s, ds, eff = M.slowness(z, x, angle)
        length = dnx * d
        col.append(z * M.nx + x)
        ln.append(length)
        tm.append(length * s)
        dt.append(length * ds)
        ef.append(eff)
        ch.append(M.christoffel(z, x))
    return col, ln, tm, dt, ef, ch


def rows(M, ray_len, xy, sg, dnx, flags=None):
    """The request's CSR and status: (row_ptr int64, col int32, len, time, dth float64, status int32)."""
    ray_len = np.asarray(ray_len, dtype=np.int64)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n = len(ray_len)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    status = np.zeros(n, dtype=np.int32)
    col, ln, tm, dt = [], [], [], []
    off = 0
    for k in range(n):
        m = max(int(ray_len[k]), 0)
        p = xy[off:off + m]
        off += m
        row_ptr[k + 1] = row_ptr[k]
        if m < 2 or (flags is not None and int(flags[k]) & 6):
            continue
        ents = [segment_entries(M, float(p[i, 0]), float(p[i + 1, 0]), float(p[i, 1]), float(p[i + 1, 1]), sg, dnx)
                for i in range(m - 1)]
        if any(e is None for e in ents):
            status[k] = 1
            continue
        for e in ents:
            col += e[0]
            ln += e[1]
            tm += e[2]
            dt += e[3]
            row_ptr[k + 1] += len(e[0])
    return (row_ptr, np.array(col, dtype=np.int32), np.array(ln, dtype=np.float64), np.array(tm, dtype=np.float64),
            np.array(dt, dtype=np.float64), status)


def maps_of(r, nz, nx, weights=None):
    """(maps (3, nz, nx), entries per cell, sum of |terms| per map and cell) of a request's rows:
    np.add.at of w * len, w * time, w * dth."""
    row_ptr, col, ln, tm, dt, _ = r
    w = np.ones(len(row_ptr) - 1) if weights is None else np.asarray(weights, dtype=np.float64)
    we = np.repeat(w, np.diff(row_ptr))
    live = we != 0.0
    out = np.zeros((3, nz * nx))
    mag = np.zeros((3, nz * nx))
    cnt = np.zeros(nz * nx, dtype=np.int64)
    np.add.at(cnt, col[live], 1)
    for q, v in enumerate((ln, tm, dt)):
        np.add.at(out[q], col[live], we[live] * v[live])
        np.add.at(mag[q], col[live], np.abs(we[live] * v[live]))
    return out.reshape(3, nz, nx), cnt.reshape(nz, nx), mag.reshape(3, nz, nx)


def write_sim_input(path, m, ray_len, xy, sg, dnx, flags=None):
    """The input file of tests/sens_sim.cpp."""
    ray_len = np.ascontiguousarray(ray_len, dtype=np.int32)
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    nz, nx = m.veln.shape
    table = np.ascontiguousarray(m.table, dtype=np.float64)
    head = np.array([nz, nx, table.shape[1], 0 if m.sd is None else 1, sg, len(ray_len), len(xy),
                     0 if flags is None else 1], dtype=np.int64)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(np.array([dnx], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(m.veln, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(m.velpn, dtype=np.int64).tobytes())
        f.write(np.ascontiguousarray(m.vm, dtype=np.float64).tobytes())
        if m.sd is not None:
            f.write(np.ascontiguousarray(m.sd, dtype=np.int64).tobytes())
        f.write(table.tobytes())
        f.write(ray_len.tobytes())
        if flags is not None:
            f.write(np.ascontiguousarray(flags, dtype=np.int32).tobytes())
        f.write(xy.tobytes())


def read_sim_output(path):
    """(row_ptr, col, len, time, dth, status) written by tests/sens_sim.cpp."""
    b = open(path, "rb").read()
    n = int(np.frombuffer(b, dtype=np.int64, count=1)[0])
    o = 8
    row_ptr = np.frombuffer(b, dtype=np.int64, count=n + 1, offset=o)
    o += 8 * (n + 1)
    status = np.frombuffer(b, dtype=np.int32, count=n, offset=o)
    o += 4 * n
    t = int(row_ptr[n])
    col = np.frombuffer(b, dtype=np.int32, count=t, offset=o)
    o += 4 * t
    out = []
    for _ in range(3):
        out.append(np.frombuffer(b, dtype=np.float64, count=t, offset=o))
        o += 8 * t
    assert o == len(b), (o, len(b))
    return row_ptr, col, out[0], out[1], out[2], status


def segments_request(segs):
    """A list of ray_cases segments as two-point rays: (ray_len, xy)."""
    xy = np.array([[(s.x1, s.y1), (s.x2, s.y2)] for s in segs], dtype=np.float64).reshape(-1, 2)
    return np.full(len(segs), 2, dtype=np.int32), xy


# segments whose walk never ends without the piece bound (horizontal at z = k + 0.5 or vertical at
# x = k + 0.5, k odd, coarse coordinates; fine coordinates = subgrid * these), and other bad input: (x1, y1, x2, y2) at subgrid 1
NEVER_ENDING = ((3.0, 1.5, 9.0, 1.5), (9.0, 3.5, 3.0, 3.5), (0.0, 5.5, 19.0, 5.5), (4.25, 7.5, 4.75, 7.5),
                (5.5, 14.0, 5.5, 3.0), (3.5, 2.0, 3.5, 2.0))
BAD_POINTS = ((float("nan"), 2.0, 5.0, 2.0), (2.0, 2.0, 5.0, float("nan")), (float("inf"), 2.0, 5.0, 2.0),
              (2.0, float("-inf"), 5.0, 2.0), (1e300, 2.0, 5.0, 2.0), (2.0, 2.0, 5.0, -1e300), (1e300, 1e300, -1e300, -1e300),
              (2.0, 2.0, 400.0, 3.0), (2.0, 2.0, 5.0, 40.0), (-400.0, 2.0, 5.0, 2.0), (2.0, 2.0, 2.0, 1e6),
              (2.0 ** 31, 2.0, 2.0 ** 31 + 3, 2.0), (1e19, 1e19, 1e19, 1e19), (2.0, 2.0, 2.0 ** 40, 2.0 ** 40))


def bad_request(sg=1):
    """Two-point rays: a good one, then every never-ending and bad segment, each followed by the good
    one; one three-point ray whose second segment never ends; rays of 0 and 1 points; a flagged ray."""
    good = (2.0 * sg, 2.0 * sg, 11.5 * sg, 7.25 * sg)
    segs = [good]
    for s in NEVER_ENDING:
        segs += [tuple(sg * v for v in s), good]
    for s in BAD_POINTS:
        segs += [tuple(sg * v for v in s), good]
    ray_len = [2] * len(segs)
    xy = [[(s[0], s[1]), (s[2], s[3])] for s in segs]
    bad = [k for k, s in enumerate(segs) if s != good]
    ray_len += [3, 0, 1, 2, 2]
    xy += [[(1.0 * sg, 1.0 * sg), (3.0 * sg, 1.5 * sg), (9.0 * sg, 1.5 * sg)], [], [(4.0, 4.0)],
           [(good[0], good[1]), (good[2], good[3])], [(good[0], good[1]), (good[2], good[3])]]
    bad.append(len(segs))
    flags = np.zeros(len(ray_len), dtype=np.int32)
    flags[-1] = 2
    flags[-2] = 1  # the early exit: a whole ray
    return (np.array(ray_len, dtype=np.int32), np.array([p for r in xy for p in r], dtype=np.float64).reshape(-1, 2),
            flags, np.array(bad))
