"""numpy restatement of the FMC modelling contract of include/alifmm.h (alifmm_tfm_model), the exact
transpose of the TFM sum (tests/tfm_ref.py), the bars of its tests, and the input file of the
stand-alone host model tests/tfm_model_sim.cpp.

One term (a, b) at a pixel p whose components are not all zero, float64, in this order: w = weight
or 1 (0: no term); u = ((T_a(p) + T_b(p)) - t0) * fs; no term unless u >= 0 and u < nt - 1;
k = int(u), f = u - k; per component g = w * refl[p][c], c1 = f * g, c0 = g - c1; c0 is added to
sample k and c1 to sample k + 1 of the pair's trace.
"""
import numpy as np

import tfm_ref as R


def noise_map(shape, ncomp=2, seed=21, keep=0.5):
    """Seeded float64 noise with about 1 - keep of its pixels set to 0: real, or complex for ncomp 2."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(tuple(shape) + (ncomp,))
    x[rng.random(tuple(shape)) >= keep] = 0.0
    return x[..., 0] if ncomp == 1 else np.ascontiguousarray(x).view(np.complex128)[..., 0]


def as_components(refl):
    """(niz, nix) real or complex -> float64 (niz, nix, ncomp)."""
    refl = np.asarray(refl)
    if np.iscomplexobj(refl):
        return np.ascontiguousarray(refl, dtype=np.complex128).view(np.float64).reshape(refl.shape + (2,))
    return np.ascontiguousarray(refl, dtype=np.float64)[..., None]


def _terms(ttx, trx, x, nt, fs, t0, weights, window, step):
    """Per transmitter a: (a, w (nrx,), ok (nrx, npix), k, f, u) over the non-zero pixels; also the
    (npix, nc) reflectivities of those pixels."""
    ttx, trx = np.asarray(ttx, dtype=np.float64), np.asarray(trx, dtype=np.float64)
    ntx, nrx = ttx.shape[0], trx.shape[0]
    assert ttx.shape[1:] == trx.shape[1:]
    if window is None:
        window = R.full_window(ttx.shape[1:], step)
    iz0, ix0, niz, nix = window
    assert x.shape[:2] == (niz, nix), (x.shape, window)
    zs, xs = iz0 + step * np.arange(niz), ix0 + step * np.arange(nix)
    assert zs[-1] < ttx.shape[1] and xs[-1] < ttx.shape[2]
    nz = np.flatnonzero((x != 0).any(axis=2).ravel())  # raster order
    pz, px = zs[nz // nix], xs[nz % nix]
    xv = x.reshape(niz * nix, -1)[nz]
    tb = trx[:, pz, px]  # (nrx, npix)
    w64 = np.ones((ntx, nrx)) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)

    def gen():
        with np.errstate(all="ignore"):
            for a in range(ntx):
                u = ((ttx[a, pz, px][None] + tb) - t0) * fs
                live = (w64[a] != 0.0)[:, None] & np.ones(u.shape, dtype=bool)
                ok = (u >= 0.0) & (u < nt - 1) & live
                k = np.where(ok, u, 0.0).astype(np.int64)
                f = u - k
                yield a, w64[a], live, ok, k, f, u

    return gen(), xv, ntx, nrx


def model_ref(ttx, trx, refl, nt, fs, t0=0.0, weights=None, window=None, step=1):
    """Returns (d, A, n, counts).  ttx (ntx, fnz, fnx), trx (nrx, fnz, fnx) float64 fields; refl
    (niz, nix) real or complex on the window.  d: float64 or complex128 (ntx, nrx, nt), every
    sample summed in the order pixel after pixel (raster), c0 before c1.  A[a][b][k] = sum over the
    contributions to that sample of |w| max_c |refl_c|: the magnitude the rounding-error bound is
    stated against.  n[a][b][k]: the number of contributions (two per in-range term, one to sample
    k and one to k + 1).  counts: terms of the non-zero pixels in range, below, above, non-finite
    and skipped by a zero weight."""
    x = as_components(refl)
    nc = x.shape[2]
    terms, xv, ntx, nrx = _terms(ttx, trx, x, nt, fs, t0, weights, window, step)
    dc = np.zeros((nc, ntx, nrx, nt))  # component-major, so that a pair of (a, c) is a contiguous view
    A = np.zeros((ntx, nrx, nt))
    n = np.zeros((ntx, nrx, nt), dtype=np.int64)
    cnt = dict(inside=0, below=0, above=0, nonfinite=0, zero_weight=0)
    xmax = np.abs(xv).max(axis=1) if len(xv) else np.zeros(0)
    for a, w, live, ok, k, f, u in terms:
        fin = np.isfinite(u)
        cnt["zero_weight"] += int((~live).sum())
        cnt["inside"] += int(ok.sum())
        cnt["nonfinite"] += int((~fin & live).sum())
        cnt["below"] += int((fin & live & (u < 0.0)).sum())
        cnt["above"] += int((fin & live & (u >= nt - 1)).sum())
        b, p = np.nonzero(ok)  # receiver-major, pixels in raster order within a receiver
        kk, ff = k[b, p], f[b, p]
        idx = np.stack([b * nt + kk, b * nt + kk + 1], axis=1).ravel()  # c0's sample, then c1's, term after term
        for c in range(nc):
            g = w[b] * xv[p, c]
            c1 = ff * g
            c0 = g - c1
            np.add.at(dc[c, a].reshape(-1), idx, np.stack([c0, c1], axis=1).ravel())
        m = np.abs(w[b]) * xmax[p]
        np.add.at(A[a].reshape(-1), idx, np.repeat(m, 2))
        np.add.at(n[a].reshape(-1), idx, 1)
    d = np.ascontiguousarray(np.moveaxis(dc, 0, -1))
    data = d.view(np.complex128)[..., 0] if nc == 2 else d[..., 0]
    return data, A, n, cnt


def bound(n, A):
    """|d - d_ref| <= 2 (n + 4) 2^-53 A, per sample and component.  Derived: g, c1 and c0 carry at
    most four roundings of magnitude <= |w refl| between them, a sum of n values in any order adds
    at most (n - 1) 2^-53 sum |value|, and both sides may deviate from the exact sum."""
    return 2.0 * (n + 4) * 2.0 ** -53 * A


def worst_ratio(d, ref, n, A):
    """max over samples and components of |d - d_ref| / bound (0 / 0 counts as 0; x / 0 as inf, so a
    sample without contributions must be exactly 0)."""
    e = np.asarray(d) - np.asarray(ref)
    err = np.maximum(np.abs(e.real), np.abs(e.imag)) if np.iscomplexobj(e) else np.abs(e)
    b = bound(n, A)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    return float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0


def inner(a, b):
    """The real inner product over samples (pixels) and components."""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.sum(a.real * b.real) + np.sum(a.imag * b.imag))


def adjoint_bar(ttx, trx, fmc, refl, fs, t0=0.0, weights=None, window=None, step=1):
    """Returns (bar, N, S) of the adjoint identity |<tfm(d), x> - <d, model(x)>| <= 2 (N + 8) 2^-53 S.
    N: the in-range terms (of the non-zero pixels); S: the sum over those terms and the components
    of |w| (|x0| + |x1|) |refl_c|, x0 and x1 the data samples k and k + 1 of the pair, d being the
    float32 data tfm() reads.

    Derivation.  Exactly, both sides are the same sum over the in-range terms and components of
    w refl_c ((1 - f) x0 + f x1).  On the imaging side a term's value times refl_c carries four
    roundings (three of tfm's term, the product), each of magnitude <= 2^-53 |w| (|x0| + |x1|)
    |refl_c|, and the N values are summed (over the pairs into the image, over the pixels into the
    inner product) in some order: at most (N - 1) 2^-53 times the sum of their magnitudes on top.
    On the modelling side g, c1, c0 and the products with x0 and x1 carry the same count of
    roundings of the same magnitude, and the sums (over the pixels into a sample, over the samples
    into the inner product) add the same again.  That is (N + 3) 2^-53 S per side; the bar takes
    N + 8 per side, which leaves room for the second-order terms and for c0 x0 and c1 x1 entering
    their sums separately where one of them dominates.  (The strict worst case of 2 N separately
    summed halves is (3 N + 7) 2^-53 S; rounding errors of random sign stay orders of magnitude
    below either, and one dropped term of typical size |w| |x| |refl| exceeds both.)"""
    x = as_components(refl)
    s = R.as_samples(fmc).astype(np.float64)
    nt = s.shape[2]
    terms, xv, ntx, nrx = _terms(ttx, trx, x, nt, fs, t0, weights, window, step)
    N, S = 0, 0.0
    for a, w, live, ok, k, f, u in terms:
        b, p = np.nonzero(ok)
        kk = k[b, p]
        N += len(b)
        mag = ((np.abs(s[a, b, kk, :]) + np.abs(s[a, b, kk + 1, :])) * np.abs(xv[p])).sum(axis=1)
        S += float(np.sum(np.abs(w[b]) * mag))
    return 2.0 * (N + 8) * 2.0 ** -53 * S, N, S


def tile_edge_fraction(ttx, trx, refl, nt, fs, t0=0.0, weights=None, window=None, step=1, tile=64):
    """The fraction of the in-range terms whose k is the last sample of a time tile of `tile`
    samples (c0 in one tile, c1 in the next): the case a tiling bug breaks."""
    terms, _, _, _ = _terms(ttx, trx, as_components(refl), nt, fs, t0, weights, window, step)
    inside = edge = 0
    for a, w, live, ok, k, f, u in terms:
        inside += int(ok.sum())
        edge += int((ok & (k % tile == tile - 1)).sum())
    return edge / max(inside, 1)


def write_sim_input(path, flds, tx, rx, refl, nt, fs, t0, weights, window, step, tile):
    """The input file of tests/tfm_model_sim.cpp: int64[16] header (ntx, nrx, nt, ncomp, nfields, fnz,
    fnx, iz0, ix0, niz, nix, step, has_weights, tile, 0, 0), float64 t0, fs, int32 tx[ntx], rx[nrx]
    (indices into the fields), float64 fields, float64 refl [niz][nix][ncomp], float32 weights."""
    flds = np.ascontiguousarray(flds, dtype=np.float64)
    x = as_components(refl)
    hdr = np.array([len(tx), len(rx), nt, x.shape[2], flds.shape[0], flds.shape[1], flds.shape[2], *window, step,
                    weights is not None, tile, 0, 0], dtype=np.int64)
    with open(path, "wb") as f:
        f.write(hdr.tobytes())
        f.write(np.array([t0, fs], dtype=np.float64).tobytes())
        f.write(np.asarray(tx, dtype=np.int32).tobytes())
        f.write(np.asarray(rx, dtype=np.int32).tobytes())
        f.write(flds.tobytes())
        f.write(x.tobytes())
        if weights is not None:
            f.write(np.ascontiguousarray(weights, dtype=np.float32).tobytes())
