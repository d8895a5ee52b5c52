"""numpy restatement of the trace FIR contract of include/alifmm.h (alifmm_trace_fir and the operator
P A of alifmm_tfm_lsq_pulse), the test pulse, the bar of the adjoint identity, and the files of the
stand-alone host program tests/trace_fir_sim.cpp.  Test infrastructure only.

fir_ref() is the definition line for line: a loop over the taps, ascending, each adding one shifted
slice; real arithmetic only (re and im are separate arrays; each product and each add is its own
numpy operation, so numpy's complex multiply never decides a rounding, and numpy never contracts).
A sample outside the trace adds nothing: the slice simply does not reach there.  So the device's
outputs equal fir_ref()'s bit for bit (np.array_equal), for any finite taps.
"""
import numpy as np

import tfm_lsq_ref as L

MAX_TAPS = 1024  # ALIFMM_FIR_MAX_TAPS


def pulse(ntap, cyc, cplx):
    """The test pulse: a Gaussian envelope (sigma = ntap / 6, centred at (ntap - 1) / 2) times a
    carrier of cyc cycles over the ntap taps, cos(phi) or exp(i phi)."""
    k = np.arange(ntap) - (ntap - 1) / 2
    env = np.exp(-0.5 * (k / (ntap / 6.0)) ** 2)
    phi = 2 * np.pi * cyc * k / ntap
    return env * np.exp(1j * phi) if cplx else env * np.cos(phi)


def _parts(a):
    """A real or complex array -> (re, im) float64, im None for a real one."""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        a = np.asarray(a, dtype=np.complex128)
        return np.ascontiguousarray(a.real), np.ascontiguousarray(a.imag)
    return np.ascontiguousarray(a, dtype=np.float64), None


def _fir(xr, xi, hr, hi, origin, transpose):
    """The sum on separate components: x (..., nt) re / im (im None: real data), taps hr / hi (hi
    None: real taps).  Returns (yr, yi)."""
    nt, ntap = xr.shape[-1], len(hr)
    assert 0 <= origin < ntap and (hi is None or xi is not None)
    yr = np.zeros(xr.shape)
    yi = None if xi is None else np.zeros(xr.shape)
    for j in range(ntap):
        # forward: y[t] += h[j] x[t - d], d = j - origin; transpose: z[t] += conj(h[j]) y[t - d], d = origin - j
        d = origin - j if transpose else j - origin
        lo, hi_t = max(0, d), min(nt, nt + d)
        if lo >= hi_t:
            continue
        dst, src = slice(lo, hi_t), slice(lo - d, hi_t - d)
        a = hr[j]
        if hi is None:
            yr[..., dst] = yr[..., dst] + a * xr[..., src]
            if xi is not None:
                yi[..., dst] = yi[..., dst] + a * xi[..., src]
        else:
            b = -hi[j] if transpose else hi[j]
            pr = (a * xr[..., src]) - (b * xi[..., src])
            pi = (a * xi[..., src]) + (b * xr[..., src])
            yr[..., dst] = yr[..., dst] + pr
            yi[..., dst] = yi[..., dst] + pi
    return yr, yi


def fir_ref(data, taps, origin=0, transpose=False):
    """P data (transpose: Pᵀ data) for data (..., nt) real or complex and a 1-D real or complex
    pulse (complex: complex data only); float64 or complex128 of data's shape."""
    xr, xi = _parts(data)
    hr, hi = _parts(taps)
    assert hr.ndim == 1 and 1 <= len(hr) <= MAX_TAPS and np.isfinite(hr).all() and (hi is None or np.isfinite(hi).all())
    with np.errstate(all="ignore"):
        yr, yi = _fir(xr, xi, hr, hi, origin, transpose)
    if yi is None:
        return yr
    out = np.empty(yr.shape, dtype=np.complex128)
    out.real, out.imag = yr, yi
    return out


def interleave(v):
    """(..., nt) real or complex -> the real vector of its components, interleaved."""
    return L.columns(v).ravel()


def dense_P(nt, taps, origin, ncomp, transpose=False):
    """The real matrix (nt ncomp, nt ncomp) of fir_ref() on one trace, its components interleaved:
    column k is fir_ref() of the k-th unit vector."""
    n = nt * ncomp
    P = np.zeros((n, n))
    e = np.zeros((nt, ncomp))
    for k in range(n):
        e.flat[k] = 1.0
        x = e.view(np.complex128)[:, 0] if ncomp == 2 else e[:, 0]
        P[:, k] = interleave(fir_ref(x, taps, origin, transpose))
        e.flat[k] = 0.0
    return P


def dense_PA(A, ntrace, nt, taps, origin, ncomp):
    """The real matrix (ntrace nt ncomp, npix ncomp) of P A on interleaved unknowns and interleaved
    data, A (ntrace nt, npix) being tfm_lsq_ref.dense_A (it acts component-wise)."""
    npix = A.shape[1]
    cols = np.ascontiguousarray(A.T).reshape(npix, ntrace, nt)
    if ncomp == 1:
        return fir_ref(cols, taps, origin).reshape(npix, -1).T.copy()
    B = np.zeros((ntrace * nt * 2, npix * 2))
    re = L.columns(fir_ref(cols + 0j, taps, origin)).reshape(npix, -1)   # P A applied to a real unit pixel
    im = L.columns(fir_ref(1j * cols, taps, origin)).reshape(npix, -1)   # ... to an imaginary one
    B[:, 0::2], B[:, 1::2] = re.T, im.T
    return B


def dense_D(D, ncomp):
    """D of the window on interleaved unknowns."""
    return D if ncomp == 1 else np.kron(D, np.eye(2))


def adjoint_bar(x, y, taps, origin):
    """(bar, S) of |<P x, y> - <x, Pᵀ y>| <= bar = 2 (ntap + M + 4) 2^-53 S for x, y (ntrace, nt), M
    their real elements, both inner products real and formed in float64.

    Derivation, in the manner of tfm_model_ref.adjoint_bar.  Exactly, both sides are the same sum
    over the outputs t, the taps j and the components of the real products h x y; S is the sum of
    their magnitudes.  On either side a term carries up to three roundings (the tap's product, the
    subtraction or addition that combines a complex tap's two products, the product with the other
    vector's element), each at most 2^-53 of the term's magnitude, and the terms are then added in
    two chains: the ntap taps of an output (or of an input, on the transposed side) and the M
    elements of the inner product, in some order, at most (ntap - 1) + (M - 1) additions, each
    adding at most 2^-53 of the sum of the magnitudes below it.  That is (ntap + M + 1) 2^-53 S per
    side; the bar takes ntap + M + 4, which leaves room for the second-order terms."""
    xr, xi = _parts(x)
    yr, yi = _parts(y)
    hr, hi = _parts(taps)
    ar = np.abs(hr)
    S = float(np.sum(_fir(np.abs(xr), None, ar, None, origin, False)[0] * np.abs(yr)))
    if xi is not None:
        S += float(np.sum(_fir(np.abs(xi), None, ar, None, origin, False)[0] * np.abs(yi)))
        if hi is not None:
            ai = np.abs(hi)
            S += float(np.sum(_fir(np.abs(xi), None, ai, None, origin, False)[0] * np.abs(yr)))
            S += float(np.sum(_fir(np.abs(xr), None, ai, None, origin, False)[0] * np.abs(yi)))
    M = xr.size * (1 if xi is None else 2)
    return 2.0 * (len(hr) + M + 4) * 2.0 ** -53 * S, S


def real_dot(a, b):
    """The real inner product of two real or complex arrays."""
    ar, ai = _parts(a)
    br, bi = _parts(b)
    return float(np.sum(ar * br)) + (0.0 if ai is None else float(np.sum(ai * bi)))


def noise(shape, cplx, seed):
    """Seeded float64 noise, real or complex."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal(shape)
    return d + 1j * rng.standard_normal(shape) if cplx else d


# ---- the shape list of the bit-equality tests (tile: the outputs a workgroup makes) ----

def shapes(tile):
    """(nt, ntap, origin) over nt in {1, 2, tile - 1, tile, tile + 1, 2 tile + 3}, ntap in {1, 2, 17,
    1024} and tile + 5 where that is a legal length (a halo longer than a tile, a pulse longer than
    the trace, the cap itself), origin in {0, ntap // 2, ntap - 1}."""
    ntaps = [1, 2, 17, MAX_TAPS] + ([tile + 5] if tile + 5 <= MAX_TAPS else [])
    out = []
    for nt in sorted({1, 2, tile - 1, tile, tile + 1, 2 * tile + 3}):
        for ntap in ntaps:
            for origin in sorted({0, ntap // 2, ntap - 1}):
                out.append((nt, ntap, origin))
    return out


TYPES = (("real_real", False, False), ("complex_real", True, False), ("complex_complex", True, True))


def noise_taps(ntap, cplx, seed=3):
    """Seeded taps of ordinary size without structure (the Gaussian test pulse underflows to
    denormals at 1024 taps: these do not)."""
    return noise(ntap, cplx, seed + ntap)


# ---- tests/trace_fir_sim.cpp ----

def write_sim_input(path, data, taps, origin, transpose, tile):
    """int64[8] header (ntrace, nt, ncomp, ntap, tap_comp, origin, transpose, tile), float64 data
    [ntrace][nt][ncomp], float64 taps [ntap][tap_comp]."""
    d, h = L.columns(data), L.columns(taps)
    nt = np.shape(data)[-1]
    hdr = np.array([np.size(data) // nt, nt, d.shape[1], h.shape[0], h.shape[1], origin, int(transpose), tile],
                   dtype=np.int64)
    with open(path, "wb") as f:
        f.write(hdr.tobytes())
        f.write(d.tobytes())
        f.write(h.tobytes())


def read_sim_output(path, like):
    """The program's output as an array of the shape and kind of `like`."""
    b = np.fromfile(path, dtype=np.float64)
    nc = 2 if np.iscomplexobj(like) else 1
    assert len(b) == np.size(like) * nc, (len(b), np.shape(like))
    return L.from_columns(b.reshape(-1, nc), np.shape(like))
