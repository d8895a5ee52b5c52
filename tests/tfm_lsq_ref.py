"""numpy restatement of the least-squares imaging contract of include/alifmm.h (alifmm_tfm_f64 and
alifmm_tfm_lsq), the cases of its tests, and the input file of the stand-alone host model
tests/tfm_lsq_sim.cpp.  Test infrastructure only.

tfm_f64_ref() is tfm_ref.tfm_ref() with the samples read as float64.  dense_A() is the linear map
of alifmm_tfm_model on the dense window as a real matrix (samples x pixels), built column by column
with tfm_model_ref.model_ref(); it acts component-wise, so a complex map or data set is an array
with a last axis of 2 here and the same matrix applies to both columns.  difference() is D of the
window.  cgls() is the iteration of the header, line for line, with the same stop rule; lstsq() is
numpy's answer on the stacked system [A; damp I; smooth D].
"""
import numpy as np

import solve_ref
import tfm_model_ref as M
import tfm_ref as R

REASONS = solve_ref.REASONS

# name -> (elements, window, step): A is 23520 x 117 (sigma 10.1 .. 4.15), 23520 x 200 (8.94 .. 3.99),
# 1920 x 117 (3.29 .. 0.47) and 480 x 117 (1.62 .. ~0, rank 106: the damping decides)
CASES = {"e7": (7, (10, 20, 9, 13), 1),
         "e7s3": (7, (4, 6, 10, 20), 3),
         "e2": (2, (10, 20, 9, 13), 1),
         "e1": (1, (10, 20, 9, 13), 1)}
NOISE = 0.01
DAMP = 1e-2  # in units of sigma_max


def as_samples64(fmc):
    """(ntx, nrx, nt) real or complex -> float64 (ntx, nrx, nt, ncomp)."""
    fmc = np.asarray(fmc)
    if np.iscomplexobj(fmc):
        return np.ascontiguousarray(fmc, dtype=np.complex128).view(np.float64).reshape(fmc.shape + (2,))
    return np.ascontiguousarray(fmc, dtype=np.float64)[..., None]


def noise64(ntx, nrx, nt=R.NT, ncomp=2, seed=6):
    """Seeded float64 noise that float32 does not represent: (ntx, nrx, nt) float64 or complex128."""
    d = np.random.default_rng(seed).standard_normal((ntx, nrx, nt, ncomp))
    assert (d.astype(np.float32).astype(np.float64) != d).mean() > 0.99
    return d[..., 0] if ncomp == 1 else np.ascontiguousarray(d).view(np.complex128)[..., 0]


def tfm_f64_ref(ttx, trx, fmc, fs, t0=0.0, weights=None, window=None, step=1):
    """tfm_ref.tfm_ref() on float64 samples: (image, A) with A(p) the magnitude of tfm_ref.bound.
    The terms of a pixel are added pair after pair (a, then b), a term out of range adding 0.0."""
    ttx, trx = np.asarray(ttx, dtype=np.float64), np.asarray(trx, dtype=np.float64)
    s = as_samples64(fmc)
    ntx, nrx, nt, nc = s.shape
    assert ttx.shape[0] == ntx and trx.shape[0] == nrx and ttx.shape[1:] == trx.shape[1:]
    if window is None:
        window = R.full_window(ttx.shape[1:], step)
    iz0, ix0, niz, nix = window
    zs, xs = iz0 + step * np.arange(niz), ix0 + step * np.arange(nix)
    assert zs[-1] < ttx.shape[1] and xs[-1] < ttx.shape[2]
    ta_all, tb_all = ttx[:, zs][:, :, xs], trx[:, zs][:, :, xs]
    img = np.zeros((niz, nix, nc))
    mag = np.zeros((niz, nix))
    w64 = np.ones((ntx, nrx)) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    rows = np.arange(nrx)[:, None, None]
    with np.errstate(all="ignore"):
        for a in range(ntx):
            live = (w64[a] != 0.0)[:, None, None]
            u = ((ta_all[a][None] + tb_all) - t0) * fs
            ok = (u >= 0.0) & (u < nt - 1) & live
            k = np.where(ok, u, 0.0).astype(np.intp)
            f = u - k
            k += rows * nt
            w = w64[a][:, None, None]
            term = np.empty(u.shape + (nc,))
            tmag = np.zeros(u.shape)
            for c in range(nc):
                sc = np.ascontiguousarray(s[a, :, :, c]).ravel()
                x0, x1 = np.take(sc, k), np.take(sc, k + 1)
                term[..., c] = np.where(ok, w * (x0 + f * (x1 - x0)), 0.0)
                np.maximum(tmag, np.abs(x0) + np.abs(x1), out=tmag)
            tmag = np.where(ok, np.abs(w) * tmag, 0.0)
            for b in range(nrx):
                img += term[b]
                mag += tmag[b]
    image = img.view(np.complex128)[..., 0] if nc == 2 else img[..., 0]
    return image, mag


def cast_gap(npairs):
    """The factor by which an image of the float32 cast of float64 noise must miss tfm_ref.bound at
    least, somewhere.  Derived: a cast moves a sample by up to 2^-25 of its magnitude, on average
    about a third of that; the npairs terms of a pixel then move its sum by about sqrt(npairs)
    2^-25 / 3 times a typical |x0| + |x1|, the worst pixel by several times that, while the bar is
    2 (npairs + 4) 2^-53 times the sum of the npairs magnitudes |x0| + |x1|.  The quotient is
    2^28 / (6 (npairs + 4) sqrt(npairs)); a quarter of it is asked for.  (No data reach a factor
    above 2^28 / (npairs + 4), every cast being off by the full half ulp in the same direction: 5e6
    at 7 x 7 pairs, 6e4 at 65 x 65.)"""
    return 2.0 ** 28 / (24.0 * (npairs + 4) * np.sqrt(npairs))


def dense_A(ttx, trx, nt, fs, t0=0.0, weights=None, window=None, step=1):
    """The real matrix (ntx nrx nt, niz nix) of the modelling map: column q is model_ref() of the
    unit map at pixel q (raster order)."""
    if window is None:
        window = R.full_window(np.shape(ttx)[1:], step)
    niz, nix = window[2:]
    A = np.zeros((len(ttx) * len(trx) * nt, niz * nix))
    x = np.zeros((niz, nix))
    for q in range(niz * nix):
        x.flat[q] = 1.0
        A[:, q] = M.model_ref(ttx, trx, x, nt, fs, t0, weights, window, step)[0].ravel()
        x.flat[q] = 0.0
    return A


def difference(niz, nix):
    """D (pairs, niz nix) of the window: one row per 4-neighbour pair of pixels."""
    return solve_ref.difference(niz, nix)


def _dot(a, b):
    return float(np.sum(a * b))


def cgls(A, D, rhs, damp, smooth, max_iter, tol):
    """CGLS from x = 0 on min |A x - rhs|² + damp² |x|² + smooth² |D x|²; rhs (rows,) or (rows, ncomp),
    A and D acting on every column.  Returns (x, info, r): info as the device's info8 with the
    reason's name, and "gammas" = [gamma_0, gamma after iteration 1, ...]; r the recurred residual."""
    d2, s2 = damp * damp, smooth * smooth
    DtD = D.T @ D

    def reg(v):
        return d2 * v + s2 * (DtD @ v)

    r = np.array(rhs, dtype=np.float64)
    x = np.zeros((A.shape[1],) + r.shape[1:])
    s = A.T @ r
    p = s.copy()
    gamma0 = gamma = _dot(s, s)
    gammas = [gamma0]
    iters, reason = 0, 1
    if gamma0 == 0.0:
        reason = 2
    else:
        for it in range(1, max_iter + 1):
            q = A @ p
            qq = _dot(q, q) + _dot(p, reg(p))
            if qq == 0.0:
                reason = 2
                break
            alpha = gamma / qq
            x = x + alpha * p
            r = r - alpha * q
            s = A.T @ r - reg(x)
            new = _dot(s, s)
            beta = new / gamma
            p = s + beta * p
            gamma = new
            gammas.append(gamma)
            iters = it
            if gamma <= tol * tol * gamma0:
                reason = 0
                break
    info = {"iterations": iters, "grad0": np.sqrt(gamma0), "grad": np.sqrt(gamma),
            "rhs_norm": float(np.linalg.norm(rhs)), "res_norm": float(np.linalg.norm(r)), "reason": REASONS[reason],
            "gammas": gammas}
    return x, info, r


def stacked(A, D, rhs, damp, smooth):
    """(B, b) of the stacked dense system [A; damp I; smooth D] x = [rhs; 0; 0]."""
    n = A.shape[1]
    rhs = np.asarray(rhs)
    B = np.vstack([A, damp * np.eye(n), smooth * D])
    return B, np.concatenate([rhs, np.zeros((n + D.shape[0],) + rhs.shape[1:])])


def lstsq(A, D, rhs, damp, smooth):
    B, b = stacked(A, D, rhs, damp, smooth)
    return np.linalg.lstsq(B, b, rcond=None)[0]


def true_gradient(A, D, rhs, damp, smooth, x):
    """(|Bᵀ(b - B x)|, |Bᵀ b|) of the stacked system."""
    B, b = stacked(A, D, rhs, damp, smooth)
    return float(np.linalg.norm(B.T @ (b - B @ x))), float(np.linalg.norm(B.T @ b))


def deviation(x, ref):
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


def columns(v):
    """A real or complex array -> float64 (size, ncomp): the vector the real operator acts on."""
    v = np.asarray(v)
    if np.iscomplexobj(v):
        return np.ascontiguousarray(v, dtype=np.complex128).view(np.float64).reshape(-1, 2)
    return np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 1)


def from_columns(c, shape):
    """The inverse of columns() for an array of `shape`."""
    c = np.ascontiguousarray(c)
    return c.view(np.complex128)[:, 0].reshape(shape) if c.shape[1] == 2 else c[:, 0].reshape(shape)


_cache = {}


def case(name):
    """dict(n, window, step, T, A, D, smax) of a solve case (computed once, never modified)."""
    if name not in _cache:
        n, window, step = CASES[name]
        T = R.fields(R.element_x(n))
        A = dense_A(T, T, R.NT, R.FS, R.T0, None, window, step)
        D = difference(*window[2:])
        sv = np.linalg.svd(A, compute_uv=False)
        for a in (T, A, D, sv):
            a.setflags(write=False)
        _cache[name] = dict(n=n, window=window, step=step, T=T, A=A, D=D, sv=sv, smax=float(sv[0]))
    return _cache[name]


def problem(name, ncomp, smooth_on=False, seed=40):
    """(case, rhs (rows, ncomp), damp, smooth): rhs = A x_true + NOISE noise, damp = DAMP sigma_max,
    smooth = damp or 0."""
    c = case(name)
    key = (name, ncomp, smooth_on, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed + 7 * ncomp)
        x_true = rng.standard_normal((c["A"].shape[1], ncomp))
        rhs = c["A"] @ x_true + NOISE * rng.standard_normal((c["A"].shape[0], ncomp))
        rhs.setflags(write=False)
        _cache[key] = rhs
    damp = DAMP * c["smax"]
    return c, _cache[key], damp, damp if smooth_on else 0.0


def data_of(c, rhs):
    """rhs (rows, ncomp) -> the data array (ntx, nrx, nt) the library takes, real or complex."""
    return from_columns(rhs, (c["n"], c["n"], R.NT))


# ---- tests/tfm_lsq_sim.cpp ----

def write_sim_input(path, flds, tx, rx, fmc, fs, t0, weights, window, step, damp, smooth, max_iter, tol):
    """int64[16] header (ntx, nrx, nt, ncomp, nfields, fnz, fnx, iz0, ix0, niz, nix, step, has_weights,
    max_iter, 0, 0), float64 t0, fs, damp, smooth, tol, int32 tx[ntx], rx[nrx] (indices into the
    fields), float64 fields, float64 data [ntx][nrx][nt][ncomp], float32 weights."""
    flds = np.ascontiguousarray(flds, dtype=np.float64)
    s = as_samples64(fmc)
    ntx, nrx, nt, nc = s.shape
    assert len(tx) == ntx and len(rx) == nrx
    hdr = np.array([ntx, nrx, nt, nc, flds.shape[0], flds.shape[1], flds.shape[2], *window, step,
                    weights is not None, max_iter, 0, 0], dtype=np.int64)
    with open(path, "wb") as f:
        f.write(hdr.tobytes())
        f.write(np.array([t0, fs, damp, smooth, tol], dtype=np.float64).tobytes())
        f.write(np.asarray(tx, dtype=np.int32).tobytes())
        f.write(np.asarray(rx, dtype=np.int32).tobytes())
        f.write(flds.tobytes())
        f.write(s.tobytes())
        if weights is not None:
            f.write(np.ascontiguousarray(weights, dtype=np.float32).tobytes())


def read_sim_output(path, nimg, ndata):
    """(Aᵀ d [nimg], the solve's x [nimg], the recurred r [ndata], info8) written by tests/tfm_lsq_sim.cpp."""
    b = np.fromfile(path, dtype=np.float64)
    assert len(b) == 2 * nimg + ndata + 8, (len(b), nimg, ndata)
    return b[:nimg], b[nimg:2 * nimg], b[2 * nimg:2 * nimg + ndata], b[2 * nimg + ndata:]
