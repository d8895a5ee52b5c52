"""numpy restatement of the sparsity-regularised imaging contract of include/alifmm.h
(alifmm_tfm_sparse), the cases of its tests, and the input file of the stand-alone host model
tests/tfm_sparse_sim.cpp.  Test infrastructure only.

The problem is F(x) = ½ |B x - d|² + ½ x·R(x) + lam Σ_p |x_p| with B = P A, R(v) = damp² v +
smooth² DᵀD v and |x_p| the modulus of pixel p over its components.  An unknown is an array
(pixels, ncomp); System wraps the dense matrices of a case so that the same code serves an operator
that acts component-wise (B (rows, pixels), the data (rows, ncomp): no pulse or a real pulse) and
one that mixes the components (a complex pulse: B the real matrix on interleaved unknowns and
interleaved data, as in test_gpu_tfm_lsq_pulse.py).  fista() is the iteration of the header, line
for line, with the same stop rule; kkt_distance() measures how far a point is from optimal without
reference to any path.

Figures of fista() on the cases below (five scatterers of modulus 1 to 3, 0.01 noise, lam = 0.1
lam_max, tol 1e-8, restart on, L the true constant), confirmed by tests/test_tfm_sparse_ref.py: see
ITERS there."""
import numpy as np

import tfm_lsq_ref as L
import tfm_ref as R
import trace_fir_ref as F

REASONS = L.REASONS
SLACK = 2.0 ** -40
MAX_DOUBLINGS = 60

# name -> (pulse, ncomp): the pulses of test_gpu_tfm_lsq_pulse.py, origin = ntap // 2
PULSES = {"r17_c1": (F.pulse(17, 3, False), 1), "r17_c2": (F.pulse(17, 3, False), 2), "c33_c2": (F.pulse(33, 5, True), 2)}


class System:
    """The dense operator of a case: B (rows, pixels) acting on every component, or, flat, the real
    matrix on interleaved unknowns and data; D likewise."""

    def __init__(self, B, D, ncomp, flat, window):
        self.B, self.D, self.ncomp, self.flat, self.window = B, D, ncomp, flat, window
        self.npix = window[2] * window[3]
        self.DtD = D.T @ D
        self._smax = None
        self.h, self.origin = None, 0  # the pulse behind B, for the calls of the library (system())

    def mul(self, v):
        """B v for v (pixels, ncomp): the data vector (rows, ncomp), or flat (rows ncomp,)."""
        return self.B @ (v.ravel() if self.flat else v)

    def tmul(self, r):
        """Bᵀ r as (pixels, ncomp)."""
        return (self.B.T @ r).reshape(self.npix, self.ncomp)

    def reg(self, v, damp, smooth):
        """R(v) as (pixels, ncomp)."""
        w = v.ravel() if self.flat else v
        return (damp * damp * w + smooth * smooth * (self.DtD @ w)).reshape(self.npix, self.ncomp)

    def rhs_of(self, data):
        """A data array of the library -> the data vector."""
        v = L.columns(data)
        return v.ravel() if self.flat else v

    @property
    def smax(self):
        if self._smax is None:
            self._smax = float(np.sqrt(np.linalg.eigvalsh(self.B.T @ self.B)[-1]))
        return self._smax

    def lipschitz(self, damp, smooth):
        """sigma_max(B)² + damp² + 8 smooth², an upper bound of |BᵀB + R|₂ (|DᵀD|₂ <= 8)."""
        return self.smax ** 2 + damp * damp + 8.0 * smooth * smooth

    def true_lipschitz(self, damp, smooth):
        """|BᵀB + R|₂ itself."""
        n = self.B.shape[1]
        return float(np.linalg.eigvalsh(self.B.T @ self.B + damp * damp * np.eye(n) + smooth * smooth * self.DtD)[-1])


def modulus(v):
    """|v_p| per pixel of v (pixels, ncomp); sqrt(re² + im²) as the device forms it."""
    return np.abs(v[:, 0]) if v.shape[1] == 1 else np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])


def _dot(a, b):
    return float(np.sum(a * b))


def prox(z, tau):
    """The group shrink of the header: m > tau: z (m - tau) / m, else +0.0."""
    m = modulus(z)
    keep = m > tau
    with np.errstate(all="ignore"):
        fac = np.where(keep, (m - tau) / m, 0.0)
    return np.where(keep[:, None], z * fac[:, None], 0.0)


def power_estimate(S, g0, damp, smooth, rounds):
    v = g0 / np.sqrt(_dot(g0, g0))
    est = 0.0
    for _ in range(rounds):
        w = S.tmul(S.mul(v)) + S.reg(v, damp, smooth)
        est = np.sqrt(_dot(w, w))
        v = w / est
    return float(est)


def fista(S, rhs, damp, smooth, lam, max_iter, tol, lipschitz=0.0, power_iters=20, restart=True):
    """FISTA with backtracking and gradient restart from x = 0, the header's iteration line for line.
    lam < 0: -lam is relative to lam_max.  Returns (x (pixels, ncomp), info): info as the device's
    info12 with the reason's name, "l0" the L the first iteration began with and "gks" = [G1, G2, ...]."""
    d = np.asarray(rhs, dtype=np.float64)
    g0 = S.tmul(d)
    G0 = np.sqrt(_dot(g0, g0))
    lam_max = float(modulus(g0).max())
    if lam < 0:
        lam = -lam * lam_max
    x = np.zeros((S.npix, S.ncomp))
    info = {"iterations": 0, "grad0": float(G0), "grad": 0.0, "rhs_norm": float(np.sqrt(_dot(d, d))), "reason": REASONS[1],
            "lam_max": lam_max, "lam": float(lam), "backtracks": 0, "restarts": 0, "l0": 0.0, "gks": []}
    go = G0 != 0.0
    Lc = float(lipschitz)
    if go and not lipschitz > 0:
        Lc = power_estimate(S, g0, damp, smooth, power_iters)
        go = np.isfinite(Lc) and Lc > 0
    if go:
        info["l0"] = Lc
    else:
        info["reason"] = REASONS[2]
    y, Bx = x, np.zeros(d.shape)
    g, fy = -g0, 0.5 * _dot(d, d) + 0.5 * 0.0
    theta, doublings = 1.0, 0
    for k in range(1, max_iter + 1 if go else 0):
        while True:
            step = 1.0 / Lc
            tau = lam * step
            xn = prox(y - step * g, tau)
            Bxn = S.mul(xn)
            rn = Bxn - d
            fn = 0.5 * _dot(rn, rn) + 0.5 * _dot(xn, S.reg(xn, damp, smooth))
            dy = xn - y
            dd = _dot(dy, dy)
            Q = (fy + _dot(g, dy)) + (0.5 * Lc) * dd
            if fn <= Q + SLACK * fy:
                break
            doublings += 1
            if doublings > MAX_DOUBLINGS:
                go = False
                break
            Lc = 2 * Lc
            info["backtracks"] += 1
        if not go:
            info["reason"] = REASONS[2]
            break
        Gk = Lc * np.sqrt(dd)
        info["gks"].append(float(Gk))
        info["grad"], info["iterations"] = float(Gk), k
        if restart and _dot(y - xn, xn - x) > 0:
            theta = 1.0
            info["restarts"] += 1
        theta1 = (1.0 + np.sqrt(1.0 + 4.0 * theta * theta)) / 2.0
        beta = (theta - 1.0) / theta1
        theta = theta1
        y = xn + beta * (xn - x)
        By = Bxn + beta * (Bxn - Bx)
        x, Bx = xn, Bxn
        if Gk <= tol * G0:
            info["reason"] = REASONS[0]
            break
        if k == max_iter:
            break
        r = By - d
        yreg = S.reg(y, damp, smooth)
        fy = 0.5 * _dot(r, r) + 0.5 * _dot(y, yreg)
        g = S.tmul(r) + yreg
    info["lipschitz"] = Lc
    info["res_norm"] = float(np.linalg.norm(d - S.mul(x)))
    info["nnz"] = int((modulus(x) != 0).sum())
    return x, info


def kkt_distance(S, rhs, damp, smooth, lam, x):
    """The 2-norm over pixels of the distance from -g to lam ∂|x_p|, g = Bᵀ(B x - d) + R(x):
    |g_p + lam x_p / |x_p|| where x_p != 0, max(|g_p| - lam, 0) where x_p = 0."""
    g = S.tmul(S.mul(x) - np.asarray(rhs)) + S.reg(x, damp, smooth)
    m = modulus(x)
    on = m != 0
    with np.errstate(all="ignore"):
        u = np.where(on[:, None], x / m[:, None], 0.0)
    dist = np.where(on, modulus(g + lam * u), np.maximum(modulus(g) - lam, 0.0))
    return float(np.sqrt(np.sum(dist * dist)))


def kkt_rounding(S, rhs, damp, smooth, x):
    """What the dense products of kkt_distance() themselves lose: the bound test_gpu_tfm_lsq.py's
    true-gradient check lives under is 2 tol |Bᵀ b| with tol 1e-8, against which a float64 product of
    n terms is off by about n 2^-53 of the magnitudes it sums.  Here n = rows + pixels, the
    magnitudes |B|ᵀ(|B| |x| + |d|) + |R| |x|; the 2-norm over the unknowns."""
    aB = np.abs(S.B)
    ax = np.abs(x.ravel() if S.flat else x)
    mag = aB.T @ (aB @ ax + np.abs(rhs)) + damp * damp * ax + smooth * smooth * (np.abs(S.DtD) @ ax)
    return float((sum(S.B.shape) + 8) * 2.0 ** -53 * np.linalg.norm(mag))


# ---- the cases ----

_cache = {}


def system(name, pk=None, ncomp=None):
    """The System of tfm_lsq_ref case `name` under pulse `pk` of PULSES (None: no pulse, `ncomp`
    components).  Computed once, never modified."""
    key = (name, pk, ncomp if pk is None else None)
    if key not in _cache:
        c = L.case(name)
        if pk is None:
            S = System(c["A"], c["D"], ncomp, False, c["window"])
        else:
            h, nc = PULSES[pk]
            flat = bool(np.iscomplexobj(h))
            B = F.dense_PA(c["A"], c["n"] ** 2, R.NT, h, len(h) // 2, 2 if flat else 1)
            B.setflags(write=False)
            S = System(B, F.dense_D(c["D"], 2) if flat else c["D"], nc, flat, c["window"])
            S.h, S.origin = h, len(h) // 2
        S.c = c
        S.pk = pk
        _cache[key] = S
    return _cache[key]


def truth(S, seed=60, count=5):
    """`count` random non-zero pixels of modulus 1 to 3 (a random sign or phase), (pixels, ncomp)."""
    rng = np.random.default_rng(seed + 7 * S.ncomp)
    x = np.zeros((S.npix, S.ncomp))
    at = rng.choice(S.npix, size=count, replace=False)
    mod = rng.uniform(1.0, 3.0, size=count)
    if S.ncomp == 1:
        x[at, 0] = mod * rng.choice([-1.0, 1.0], size=count)
    else:
        ph = rng.uniform(0, 2 * np.pi, size=count)
        x[at, 0], x[at, 1] = mod * np.cos(ph), mod * np.sin(ph)
    return x


def problem(name, pk=None, ncomp=None, damp_on=False, smooth_on=False, seed=60):
    """(S, rhs, damp, smooth, x_true): rhs = B x_true + 0.01 noise, damp = 1e-2 sigma_max(B) or 0,
    smooth = 1e-2 sigma_max(B) or 0."""
    S = system(name, pk, ncomp)
    key = (name, pk, S.ncomp, seed, "rhs")
    if key not in _cache:
        xt = truth(S, seed)
        clean = S.mul(xt)
        rhs = clean + L.NOISE * np.random.default_rng(seed + 1).standard_normal(clean.shape)
        rhs.setflags(write=False)
        xt.setflags(write=False)
        _cache[key] = (rhs, xt)
    rhs, xt = _cache[key]
    a = L.DAMP * S.smax
    return S, rhs, a if damp_on else 0.0, a if smooth_on else 0.0, xt


def data_of(S, rhs):
    """A data vector of the system -> the data array (n, n, nt) the library takes."""
    return L.data_of(S.c, np.asarray(rhs).reshape(-1, S.ncomp))


# ---- tests/tfm_sparse_sim.cpp ----

def write_sim_input(path, S, rhs, damp, smooth, lam, lipschitz, power_iters, restart, max_iter, tol):
    """int64[8] header (niz, nix, ncomp, ndata, power_iters, restart, max_iter, 0), float64 damp,
    smooth, lam, lipschitz, tol, then float64 the matrix of B on interleaved unknowns and interleaved
    data [ndata][nimg] and the data [ndata]."""
    Bf = S.B if S.flat or S.ncomp == 1 else np.kron(S.B, np.eye(S.ncomp))
    d = np.ascontiguousarray(rhs, dtype=np.float64).ravel()
    assert Bf.shape == (d.size, S.npix * S.ncomp)
    hdr = np.array([S.window[2], S.window[3], S.ncomp, d.size, power_iters, int(restart), max_iter, 0], dtype=np.int64)
    with open(path, "wb") as f:
        f.write(hdr.tobytes())
        f.write(np.array([damp, smooth, lam, lipschitz, tol], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(Bf, dtype=np.float64).tobytes())
        f.write(d.tobytes())


def read_sim_output(path, S, ndata):
    """(x (pixels, ncomp), resid [ndata], info12, l0) written by tests/tfm_sparse_sim.cpp."""
    b = np.fromfile(path, dtype=np.float64)
    ni = S.npix * S.ncomp
    assert len(b) == ni + ndata + 13, (len(b), ni, ndata)
    return b[:ni].reshape(S.npix, S.ncomp), b[ni:ni + ndata], b[ni + ndata:ni + ndata + 12], b[-1]
