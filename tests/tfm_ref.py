"""numpy restatement of the TFM contract of include/alifmm.h (alifmm_tfm), the synthetic inputs of
the TFM tests, and the input file of the stand-alone host model tests/tfm_sim.cpp.

One term (a, b) at pixel p, float64, in this order: w = weight or 1 (0: no term);
u = ((T_a(p) + T_b(p)) - t0) * fs; no term unless u >= 0 and u < nt - 1; k = int(u), f = u - k;
term = w * (x0 + f * (x1 - x0)) with x0, x1 = samples k, k + 1 of the pair's A-scan.
"""
import numpy as np

# the synthetic case: 37 x 70 grid, elements on row 0, straight rays at 5000 m/s
NZ, NX, DNX, SPEED = 37, 70, 1e-3, 5000.0
FS, T0, NT = 25e6, 4e-6, 480
WINDOW = (3, 5, 29, 61)       # aligned to no tile
WINDOW_STEP3 = (1, 2, 12, 23)  # at step 3


def element_x(n, lo=2, hi=67):
    return np.round(np.linspace(lo, hi, n)).astype(int)


def fields(xs, nz=NZ, nx=NX, dnx=DNX, zs=0):
    """T_e(p) = |p - e| dnx / 5000 for elements at nodes (zs, xs[e]): (len(xs), nz, nx) float64."""
    z, x = np.mgrid[0:nz, 0:nx]
    return np.stack([np.hypot(z - zs, x - xe) * dnx / SPEED for xe in xs])


def data(ntx, nrx, nt=NT, ncomp=2, seed=5):
    """Seeded float32 noise: (ntx, nrx, nt) float32, or complex64 for ncomp 2."""
    d = np.random.default_rng(seed).standard_normal((ntx, nrx, nt, ncomp)).astype(np.float32)
    return d[..., 0] if ncomp == 1 else d.view(np.complex64)[..., 0]


def scatterer_data(tq_tx, tq_rx, fs, nt, t0=0.0):
    """Analytic echo of a point scatterer: s_ab(t) = exp(-2 (fc (t - tau))^2) exp(2 pi i fc (t - tau)),
    tau_ab = tq_tx[a] + tq_rx[b], fc = fs / 5.  complex64 (ntx, nrx, nt)."""
    fc = fs / 5
    t = t0 + np.arange(nt) / fs
    d = t[None, None, :] - (np.asarray(tq_tx)[:, None, None] + np.asarray(tq_rx)[None, :, None])
    return (np.exp(-2 * (fc * d) ** 2) * np.exp(2j * np.pi * fc * d)).astype(np.complex64)


def as_samples(fmc):
    """(ntx, nrx, nt) real or complex -> the library's float32 (ntx, nrx, nt, ncomp)."""
    fmc = np.asarray(fmc)
    if np.iscomplexobj(fmc):
        return np.ascontiguousarray(fmc, dtype=np.complex64).view(np.float32).reshape(fmc.shape + (2,))
    return np.ascontiguousarray(fmc, dtype=np.float32)[..., None]


def full_window(shape, step=1):
    return (0, 0, (shape[0] - 1) // step + 1, (shape[1] - 1) // step + 1)


def tfm_ref(ttx, trx, fmc, fs, t0=0.0, weights=None, window=None, step=1):
    """Returns (image, A, counts).  ttx (ntx, fnz, fnx), trx (nrx, fnz, fnx) float64 fields; fmc
    (ntx, nrx, nt) real or complex.  image: float64 or complex128 (niz, nix).  A(p) = sum over the
    in-range terms of |w| (|x0| + |x1|), of the larger component for complex data: the magnitude
    the rounding-error bound is stated against.  counts: terms in range, below, above,
    non-finite, and skipped by a zero weight."""
    ttx, trx = np.asarray(ttx, dtype=np.float64), np.asarray(trx, dtype=np.float64)
    s = as_samples(fmc)
    ntx, nrx, nt, nc = s.shape
    assert ttx.shape[0] == ntx and trx.shape[0] == nrx and ttx.shape[1:] == trx.shape[1:]
    if window is None:
        window = full_window(ttx.shape[1:], step)
    iz0, ix0, niz, nix = window
    zs, xs = iz0 + step * np.arange(niz), ix0 + step * np.arange(nix)
    assert zs[-1] < ttx.shape[1] and xs[-1] < ttx.shape[2]
    ta_all, tb_all = ttx[:, zs][:, :, xs], trx[:, zs][:, :, xs]
    img = np.zeros((niz, nix, nc))
    mag = np.zeros((niz, nix))
    cnt = dict(inside=0, below=0, above=0, nonfinite=0, zero_weight=0)
    w64 = np.ones((ntx, nrx)) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    rows = np.arange(nrx)[:, None, None]
    with np.errstate(all="ignore"):
        for a in range(ntx):
            # the terms of transmitter a with every receiver, pixels vectorised: (nrx, niz, nix[, nc])
            live = (w64[a] != 0.0)[:, None, None]
            u = ((ta_all[a][None] + tb_all) - t0) * fs
            ok = (u >= 0.0) & (u < nt - 1) & live
            fin = np.isfinite(u)
            cnt["zero_weight"] += int((~live).sum()) * niz * nix
            cnt["inside"] += int(ok.sum())
            cnt["nonfinite"] += int((~fin & live).sum())
            cnt["below"] += int((fin & live & (u < 0.0)).sum())
            cnt["above"] += int((fin & live & (u >= nt - 1)).sum())
            k = np.where(ok, u, 0.0).astype(np.intp)
            f = u - k
            k += rows * nt  # sample k of receiver b in the transmitter's (nrx * nt) samples
            w = w64[a][:, None, None]
            term = np.empty(u.shape + (nc,))
            tmag = np.zeros(u.shape)
            for c in range(nc):
                sc = np.ascontiguousarray(s[a, :, :, c], dtype=np.float64).ravel()
                x0, x1 = np.take(sc, k), np.take(sc, k + 1)
                term[..., c] = np.where(ok, w * (x0 + f * (x1 - x0)), 0.0)
                np.maximum(tmag, np.abs(x0) + np.abs(x1), out=tmag)
            tmag = np.where(ok, np.abs(w) * tmag, 0.0)
            for b in range(nrx):  # the sum itself: pair after pair, a term out of range adds 0.0
                img += term[b]
                mag += tmag[b]
    image = img.view(np.complex128)[..., 0] if nc == 2 else img[..., 0]
    return image, mag, cnt


def bound(npairs, mag):
    """|I - I_ref| <= 2 (npairs + 4) 2^-53 A(p), per pixel and component.  Derived: a term carries
    three float64 roundings of magnitude <= |w| (|x0| + |x1|), and a sum of n terms in any order
    adds at most (n - 1) 2^-53 sum |term|."""
    return 2.0 * (npairs + 4) * 2.0 ** -53 * mag


def worst_ratio(img, ref, npairs, mag):
    """max over pixels and components of |I - I_ref| / bound (0 / 0 counts as 0; x / 0 as inf)."""
    d = np.asarray(img) - np.asarray(ref)
    err = np.maximum(np.abs(d.real), np.abs(d.imag)) if np.iscomplexobj(d) else np.abs(d)
    b = bound(npairs, mag)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    return float(np.nan_to_num(r, nan=np.inf).max())


def write_sim_input(path, flds, tx, rx, fmc, fs, t0, weights, window, step):
    """The input file of tests/tfm_sim.cpp: int64[16] header (ntx, nrx, nt, ncomp, nfields, fnz, fnx,
    iz0, ix0, niz, nix, step, has_weights, 0, 0, 0), float64 t0, fs, int32 tx[ntx], rx[nrx] (indices
    into the fields), float64 fields, float32 data [ntx][nrx][nt][ncomp], float32 weights."""
    flds = np.ascontiguousarray(flds, dtype=np.float64)
    s = as_samples(fmc)
    ntx, nrx, nt, nc = s.shape
    assert len(tx) == ntx and len(rx) == nrx
    hdr = np.array([ntx, nrx, nt, nc, flds.shape[0], flds.shape[1], flds.shape[2], *window, step,
                    weights is not None, 0, 0, 0], dtype=np.int64)
    with open(path, "wb") as f:
        f.write(hdr.tobytes())
        f.write(np.array([t0, fs], dtype=np.float64).tobytes())
        f.write(np.asarray(tx, dtype=np.int32).tobytes())
        f.write(np.asarray(rx, dtype=np.int32).tobytes())
        f.write(flds.tobytes())
        f.write(s.tobytes())
        if weights is not None:
            f.write(np.ascontiguousarray(weights, dtype=np.float32).tobytes())
