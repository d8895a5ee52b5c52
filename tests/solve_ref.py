"""The contract of alifmm_sens_op_build / _apply / _solve (include/alifmm.h) restated in numpy: the
reference the device kernels (csrc/sens_solve.hip) and the host run of their sums
(tests/solve_sim.cpp) are tested against.  Test infrastructure only.

The operator is dense here: A[k, c] = cs[c] * (sum of the entries of ray k in cell c), from the rows
of sens_ref.rows().  D is the first difference over every 4-neighbour pair of cells that both have
cs != 0.  cgls() is the iteration of the header, line for line, with the same stop rule; lstsq() is
numpy's answer on the stacked system [A; damp I; smooth D].

awkward_request() builds the synthetic rays whose operator has the shapes the kernels treat
differently: rows of 0, 1, 2, 63, 64, 65, 255, 256, 257 and more than 1024 entries, columns of 0, 1,
4, 5, 64, 65, 256, 257 and more than 256 entries (the column product's classes end at 4 and 256
entries, a wavefront has 64 lanes, a workgroup 256).
"""
import numpy as np

REASONS = ("tol", "max_iter", "breakdown")

ROW_COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1100)
COL_COUNTS = (0, 1, 4, 5, 64, 65, 256, 257)
NZ, NX = 21, 72            # the awkward request's grid (72 columns of the stif65 stripes: all 65 rows)
FAN_CELL = (9, 36)         # the cell a fan of FAN_RAYS rays leaves
FAN_RAYS = 300


def dense(rows, quantity, ncell, cs=None):
    """A (nrays, ncell) of one quantity (0 len, 1 time, 2 dth) of a request's rows (sens_ref.rows)."""
    row_ptr, col = rows[0], rows[1]
    val = rows[2 + quantity]
    A = np.zeros((len(row_ptr) - 1, ncell))
    k = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    np.add.at(A, (k, col), val)
    return A if cs is None else A * np.asarray(cs, dtype=np.float64).ravel()[None, :]


def products(rows, quantity, ncell, cs, x, y):
    """Both products entry by entry with the contract's own terms, val * (cs[col] * x[col]) and
    cs[c] * sum(val * y[row]), added in entry order (np.add.at), so that only the order of the sums
    differs from the device's: (A x, sum |terms| per row, Aᵀ y, sum |terms| per column)."""
    row_ptr, col = rows[0], rows[1]
    val = rows[2 + quantity]
    k = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    c1 = np.ones(ncell) if cs is None else np.asarray(cs, dtype=np.float64).ravel()
    t = val * (c1[col] * x[col])
    ax, ax_mag = np.zeros(len(row_ptr) - 1), np.zeros(len(row_ptr) - 1)
    np.add.at(ax, k, t)
    np.add.at(ax_mag, k, np.abs(t))
    u = val * y[k]
    aty, aty_mag = np.zeros(ncell), np.zeros(ncell)
    np.add.at(aty, col, u)
    np.add.at(aty_mag, col, np.abs(u))
    return ax, ax_mag, c1 * aty, np.abs(c1) * aty_mag


def difference(nz, nx, cs=None):
    """D (pairs, nz * nx): one row per 4-neighbour pair of cells that both have cs != 0."""
    live = np.ones(nz * nx, dtype=bool) if cs is None else (np.asarray(cs).ravel() != 0)
    idx = np.arange(nz * nx).reshape(nz, nx)
    pairs = [(a, b) for a, b in zip(idx[:, :-1].ravel(), idx[:, 1:].ravel())]
    pairs += [(a, b) for a, b in zip(idx[:-1, :].ravel(), idx[1:, :].ravel())]
    pairs = [(a, b) for a, b in pairs if live[a] and live[b]]
    D = np.zeros((len(pairs), nz * nx))
    for i, (a, b) in enumerate(pairs):
        D[i, a], D[i, b] = 1.0, -1.0
    return D


def cgls(A, D, rhs, damp, smooth, max_iter, tol):
    """CGLS from x = 0 on min |A x - rhs|² + damp² |x|² + smooth² |D x|² without an augmented
    residual.  Returns (x, info): info as the device's info8 with the reason's name."""
    d2, s2 = damp * damp, smooth * smooth
    DtD = D.T @ D

    def reg(v):
        return d2 * v + s2 * (DtD @ v)

    x = np.zeros(A.shape[1])
    r = np.array(rhs, dtype=np.float64)
    s = A.T @ r
    p = s.copy()
    gamma0 = gamma = float(s @ s)
    iters, reason = 0, 1
    if gamma0 == 0.0:
        reason = 2
    else:
        for it in range(1, max_iter + 1):
            q = A @ p
            qq = float(q @ q + p @ reg(p))
            if qq == 0.0:
                reason = 2
                break
            alpha = gamma / qq
            x = x + alpha * p
            r = r - alpha * q
            s = A.T @ r - reg(x)
            new = float(s @ s)
            beta = new / gamma
            p = s + beta * p
            gamma = new
            iters = it
            if gamma <= tol * tol * gamma0:
                reason = 0
                break
    return x, {"iterations": iters, "grad0": np.sqrt(gamma0), "grad": np.sqrt(gamma),
               "rhs_norm": float(np.linalg.norm(rhs)), "res_norm": float(np.linalg.norm(r)), "reason": REASONS[reason]}


def stacked(A, D, rhs, damp, smooth):
    """(B, b) of the stacked dense system [A; damp I; smooth D] x = [rhs; 0; 0]."""
    n = A.shape[1]
    B = np.vstack([A, damp * np.eye(n), smooth * D])
    return B, np.concatenate([rhs, np.zeros(n + D.shape[0])])


def lstsq(A, D, rhs, damp, smooth):
    B, b = stacked(A, D, rhs, damp, smooth)
    return np.linalg.lstsq(B, b, rcond=None)[0]


def true_gradient(A, D, rhs, damp, smooth, x):
    """(|Bᵀ(b - B x)|, |Bᵀ b|) of the stacked system."""
    B, b = stacked(A, D, rhs, damp, smooth)
    return float(np.linalg.norm(B.T @ (b - B @ x))), float(np.linalg.norm(B.T @ b))


# ---- the awkward request ----

def model(name):
    """The ray_cases model `name` on the NZ x NX grid; the stripe models (stif65: 65 stiffness rows,
    past the fill kernel's LDS tables) are the first NX columns of their 21 x 300 grid."""
    import ray_cases as RC

    if name in ("iso", "grain", "mixed"):
        return RC.model(name, NZ, NX)
    m = RC.model(name, *RC.SEG_H)
    assert m.nz == NZ
    crop = [None if a is None else np.ascontiguousarray(a[:, :NX]) for a in (m.veln, m.velpn, m.vm, m.sd, m.ids)]
    return RC.Model(name, NZ, NX, crop[0], crop[1], crop[2], crop[3], m.table, crop[4])


def _tiny(z, x, k):
    """A two-point ray inside cell (z, x): one entry."""
    d = 0.002 * (k % 100)
    return [(x + 0.1 + d, z + 0.1), (x + 0.3, z + 0.2 + d / 2)]


def _zigzag(z, target):
    """A ray going back and forth along the line at depth z (a horizontal segment over m cell edges has
    m + 1 pieces) until it has `target` entries: base segments of 16 pieces, the rest split in two."""
    counts, left = [], target
    if target < 17:
        counts = [target]
    else:
        while left > 32:
            counts.append(16)
            left -= 16
        counts += [left // 2, left - left // 2]
    x, pts = 2.0, [(2.0, z)]
    for c in counts:
        m = c - 1
        x = x + m if x + m <= 38 and x <= 23 else x - m
        assert 0 <= x <= 39
        pts.append((x, z))
    return pts


def awkward_request(sg=1):
    """(ray_len int32, xy (points, 2) on the fine grid of sg, flags int32, spec): spec = dict(rows =
    {entry count: ray}, cols = {entry count: cell index}, fan = cell index, twice = a ray that visits
    a cell twice, invalid / flagged / short = the rays with empty rows)."""
    rays, spec = [], {"rows": {}, "cols": {}}
    # the tiny rays lie in row 0 of the grid, which nothing else crosses
    for i, n in enumerate(c for c in COL_COUNTS if c > 0):
        z, x = 0, 1 + 2 * i
        spec["cols"][n] = z * NX + x
        rays += [_tiny(z, x, k) for k in range(n)]
    spec["rows"][1] = 0
    spec["cols"][0] = (NZ - 1) * NX + NX - 1
    # the fan: FAN_RAYS rays leaving one cell, 6 cells long
    fz, fx = FAN_CELL
    spec["fan"] = fz * NX + fx
    for k in range(FAN_RAYS):
        th = 2 * np.pi * (k + 0.37) / FAN_RAYS
        rays.append([(fx + 0.05, fz - 0.05), (fx + 6 * np.cos(th), fz + 6 * np.sin(th))])
    # the long rows, one line each
    for i, n in enumerate(c for c in ROW_COUNTS if c > 1):
        spec["rows"][n] = len(rays)
        rays.append(_zigzag(2.25 if n == 2 else 13.25 + i, n))
    spec["twice"] = spec["rows"][63]
    # empty rows: a flagged ray, a ray of one point, an invalid ray
    spec["flagged"], spec["short"], spec["invalid"] = len(rays), len(rays) + 1, len(rays) + 2
    rays += [_tiny(1, 1, 0), [(5.0, 1.0)], [(3.0, 1.0), (float("nan"), 1.0)]]
    flags = np.zeros(len(rays), dtype=np.int32)
    flags[spec["flagged"]] = 2
    ray_len = np.array([len(r) for r in rays], dtype=np.int32)
    xy = float(sg) * np.array([p for r in rays for p in r], dtype=np.float64)
    return ray_len, xy, flags, spec


def check_awkward(row_ptr, col, status, spec):
    """The counts the request was built for really occur (asserted from row_ptr and a column
    histogram)."""
    n = np.diff(row_ptr)
    hist = np.bincount(col, minlength=NZ * NX)
    for want, k in spec["rows"].items():
        assert n[k] == want, ("row", k, want, int(n[k]))
    for k in (spec["flagged"], spec["short"], spec["invalid"]):
        assert n[k] == 0, ("empty row", k, int(n[k]))
    assert status[spec["invalid"]] == 1 and status.sum() == 1
    assert set(ROW_COUNTS[:-1]) <= set(n.tolist()) and n.max() > 1024
    for want, c in spec["cols"].items():
        assert hist[c] == want, ("column", c, want, int(hist[c]))
    assert hist[spec["fan"]] > 256
    k = spec["twice"]
    cells = col[row_ptr[k]:row_ptr[k + 1]]
    assert len(np.unique(cells)) < len(cells)


def col_scale(seed=3):
    """A column scale with zeros, negative values and values far from 1."""
    rng = np.random.default_rng(seed)
    cs = rng.choice([0.0, -2.5, 1.0e3, 1.0e-3, 1.0, 0.5, -40.0], size=(NZ, NX), p=[0.15, 0.15, 0.1, 0.1, 0.2, 0.2, 0.1])
    return cs


def rank_scale(spec, rows, quantity=1):
    """A column scale that leaves free only the tiny rays' cells and the cells within 2 cells of the
    fan's, each scaled to a column norm of 1e-3: A restricted to the free cells has full column rank
    (20 columns for the times of the mixed model)."""
    free = np.zeros((NZ, NX), dtype=bool)
    for n, c in spec["cols"].items():
        free.flat[c] = n > 0
    zz, xx = np.mgrid[0:NZ, 0:NX]
    free |= np.hypot(zz - FAN_CELL[0], xx - FAN_CELL[1]) <= 2.0
    norm = np.linalg.norm(dense(rows, quantity, NZ * NX), axis=0).reshape(NZ, NX)
    cs = np.zeros((NZ, NX))
    cs[free] = 1e-3 / norm[free]
    return cs


def block_scale(seed=4):
    """A column scale that leaves free the block of rows 0 .. 2 and columns 0 .. 8 (cells of the tiny
    rays, of the two-entry row, and cells between them that only the smoothing reaches)."""
    cs = np.zeros((NZ, NX))
    cs[0:3, 0:9] = np.random.default_rng(seed).choice([-2.5, 1.0, 0.5, 3.0], size=(3, 9))
    return cs


# The solve's cases: name -> (column scale, damp and smooth in units of |A|_F / sqrt(nrays)).  Each is
# conditioned well enough that the restatement's iteration count is decided by a wide margin (its
# gradient is at least twice the stop's threshold one iteration earlier and at most half of it at the
# stop, tests/test_solve_ref.py), so a count can be compared across summation orders: with the wide
# col_scale() a damp of 0.1 units takes 60 iterations whose count moves by 1 between two BLAS builds.
SOLVE_CASES = {"damp": (lambda spec, rows: col_scale(), 10.0, 0.0),
               "rank": (rank_scale, 0.0, 0.0),
               "smooth": (lambda spec, rows: block_scale(), 0.0, 30.0)}


def solve_case(rows, spec, name, quantity=1, seed=1):
    """(cs, A, D, rhs, damp, smooth) of a solve case on a request's reference rows."""
    scale, df, sf = SOLVE_CASES[name]
    cs = scale(spec, rows)
    A = dense(rows, quantity, NZ * NX, cs)
    D = difference(NZ, NX, cs)
    unit = float(np.linalg.norm(A)) / np.sqrt(A.shape[0])
    rhs = 1e-8 * np.random.default_rng(seed).normal(size=A.shape[0])
    return cs, A, D, rhs, df * unit, sf * unit


def deviation(x, ref):
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


# ---- tests/solve_sim.cpp ----

def write_sim_input(path, rows, quantity, nz, nx, cs, xin, yin, rhs, damp, smooth, max_iter, tol):
    row_ptr = np.ascontiguousarray(rows[0], dtype=np.int64)
    col = np.ascontiguousarray(rows[1], dtype=np.int32)
    val = np.ascontiguousarray(rows[2 + quantity], dtype=np.float64)
    head = np.array([len(row_ptr) - 1, nz, nx, len(col), 0 if cs is None else 1, max_iter], dtype=np.int64)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(np.array([damp, smooth, tol], dtype=np.float64).tobytes())
        f.write(row_ptr.tobytes())
        f.write(col.tobytes())
        f.write(val.tobytes())
        if cs is not None:
            f.write(np.ascontiguousarray(cs, dtype=np.float64).tobytes())
        for v in (xin, yin, rhs):
            f.write(np.ascontiguousarray(v, dtype=np.float64).tobytes())


def read_sim_output(path, nrays, ncell):
    """(A x, Aᵀ y, the solve's x, info8) written by tests/solve_sim.cpp."""
    b = np.fromfile(path, dtype=np.float64)
    assert len(b) == nrays + 2 * ncell + 8, (len(b), nrays, ncell)
    return b[:nrays], b[nrays:nrays + ncell], b[nrays + ncell:nrays + 2 * ncell], b[nrays + 2 * ncell:]
