"""numpy restatement of the coherence-weighted TFM contract of include/alifmm.h (alifmm_tfm_coh), on
the helpers of tests/tfm_ref.py, the error bars of its tests, and the demonstration case.

A counting term is a term of alifmm_tfm with w != 0 and 0 <= u < nt - 1; t_c is its value per
component.  Per pixel, float64, operations in this order: S_c = sum t_c (the image), n = the number
of counting terms, and
  kind 1 (CF):  e = t_0 t_0 (+ t_1 t_1), q += e;  F = n q > 0 ? (S_0 S_0 (+ S_1 S_1)) / (n q) : 0
  kind 2 (SCF): b += (t_0 > 0) - (t_0 < 0);  m = b / n, F = n > 0 ? 1 - sqrt(1 - m m) : 0
  kind 3 (PCF): g = sqrt(e); if g > 0: ph_c += t_c (1 / g);  y = max(1 - (ph_0 ph_0 + ph_1 ph_1) / (n n), 0),
                F = n > 0 ? 1 - sqrt(y) : 0
sums = (n, q, 0), (n, b, 0) or (n, ph_0, ph_1).
"""
import numpy as np

import tfm_ref as R

KINDS = {"cf": 1, "scf": 2, "pcf": 3}
U = 2.0 ** -53


def factor_of(kind, image, sums):
    """The contract's formula on an image (real or complex (niz, nix)) and raw sums (niz, nix, 3),
    every operation a correctly rounded float64 one in the contract's order."""
    kind = KINDS.get(kind, kind)
    n, x0, x1 = sums[..., 0], sums[..., 1], sums[..., 2]
    with np.errstate(all="ignore"):
        if kind == 1:
            num = image.real * image.real
            if np.iscomplexobj(image):
                num = num + image.imag * image.imag
            den = n * x0
            return np.where(den > 0, num / den, 0.0)
        if kind == 2:
            m = x0 / n
            y = 1.0 - m * m
        else:
            num = x0 * x0 + x1 * x1
            y = 1.0 - num / (n * n)
            y = np.where(y < 0, 0.0, y)
        return np.where(n > 0, 1.0 - np.sqrt(y), 0.0)


def tfm_coh_ref(ttx, trx, fmc, fs, kind, t0=0.0, weights=None, window=None, step=1):
    """Returns (image, factor, sums, mag): image and mag as tfm_ref() gives them (the same bits: the
    same terms in the same order, pair after pair), factor (niz, nix), sums (niz, nix, 3)."""
    kind = KINDS.get(kind, kind)
    ttx, trx = np.asarray(ttx, dtype=np.float64), np.asarray(trx, dtype=np.float64)
    s = R.as_samples(fmc)
    ntx, nrx, nt, nc = s.shape
    assert kind in (1, 2, 3) and (kind != 3 or nc == 2)
    assert ttx.shape[0] == ntx and trx.shape[0] == nrx and ttx.shape[1:] == trx.shape[1:]
    if window is None:
        window = R.full_window(ttx.shape[1:], step)
    iz0, ix0, niz, nix = window
    zs, xs = iz0 + step * np.arange(niz), ix0 + step * np.arange(nix)
    ta_all, tb_all = ttx[:, zs][:, :, xs], trx[:, zs][:, :, xs]
    img = np.zeros((niz, nix, nc))
    mag = np.zeros((niz, nix))
    sums = np.zeros((niz, nix, 3))
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
            t = np.empty(u.shape + (nc,))
            tmag = np.zeros(u.shape)
            for c in range(nc):
                sc = np.ascontiguousarray(s[a, :, :, c], dtype=np.float64).ravel()
                x0, x1 = np.take(sc, k), np.take(sc, k + 1)
                t[..., c] = w * (x0 + f * (x1 - x0))
                np.maximum(tmag, np.abs(x0) + np.abs(x1), out=tmag)
            tmag = np.where(ok, np.abs(w) * tmag, 0.0)
            ext = np.zeros(u.shape + (2,))
            if kind == 2:
                ext[..., 0] = (t[..., 0] > 0).astype(np.float64) - (t[..., 0] < 0)
            else:
                e = t[..., 0] * t[..., 0]
                if nc == 2:
                    e = e + t[..., 1] * t[..., 1]
                if kind == 1:
                    ext[..., 0] = e
                else:
                    g = np.sqrt(e)
                    r = 1.0 / g
                    for c in range(2):
                        ext[..., c] = np.where(g > 0, t[..., c] * r, 0.0)
            term = np.where(ok[..., None], t, 0.0)
            ext = np.where(ok[..., None], ext, 0.0)
            for b in range(nrx):  # the sums themselves: pair after pair, a term out of range adds 0.0
                img += term[b]
                mag += tmag[b]
                sums[..., 0] += ok[b]
                sums[..., 1:] += ext[b]
    image = img.view(np.complex128)[..., 0] if nc == 2 else img[..., 0]
    return image, factor_of(kind, image, sums), sums, mag


# The bars.  Every term is the same float64 number in numpy and in the code under test (no
# operation is contracted, each is correctly rounded); only the order of the sums differs.  A sum of
# n non-negative terms (q) in any order is within (n - 1) u of the exact sum relatively, u = 2^-53,
# so two orders differ by at most 2 (n - 1) u q: the bar 2 (npairs + 4) u q_ref covers it.  A term
# of ph has magnitude <= 1 (+ 2 u), so sum |term| <= n and the same argument gives
# 2 (npairs + 4) u n per component.  n and b are sums of small integers: exact.
def eps(npairs):
    return 2.0 * (npairs + 4) * U


def sums_ratio(kind, sums, ref, npairs):
    """n and b must be equal; returns the worst |x - x_ref| / bar over q or ph (0 / 0 counts as 0)."""
    kind = KINDS.get(kind, kind)
    assert sums.shape == ref.shape and np.array_equal(sums[..., 0], ref[..., 0])
    if kind == 2:
        assert np.array_equal(sums, ref)
        return 0.0
    if kind == 1:
        assert not sums[..., 2].any()
        err, bar = np.abs(sums[..., 1] - ref[..., 1]), eps(npairs) * ref[..., 1]
    else:
        err = np.abs(sums[..., 1:] - ref[..., 1:]).max(axis=-1)
        bar = eps(npairs) * ref[..., 0]
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    return float(np.nan_to_num(r, nan=np.inf).max())


def factor_bar(kind, ref_image, ref_sums, npairs, mag):
    """|F - F_ref| where F comes from sums within the bars above and an image within tfm_ref.bound
    of the reference's.  Kind 1: F = num / den; |num1/den1 - num2/den2| <= |num1 - num2| / den1 +
    F2 |den2 - den1| / den1, with |num1 - num2| <= sum_c (2 |S_c| + d) d, d = bound(npairs, mag), and
    |den2 - den1| / den1 <= eps / (1 - eps) <= 2 eps; 8 u F for the formula's own roundings on both
    sides.  Kind 2: n and b are exact and every operation is correctly rounded: 0.  Kind 3:
    y = 1 - num / n², |num1 - num2| <= sum_c (2 |ph_c| + d) d with d = eps n, 8 u for the roundings
    of y (num / n² and y are at most about 1), and |sqrt(y1) - sqrt(y2)| <= sqrt(|y1 - y2|); 4 u
    for the square root's and the subtraction's own roundings."""
    kind = KINDS.get(kind, kind)
    n = ref_sums[..., 0]
    e = eps(npairs)
    with np.errstate(all="ignore"):
        if kind == 2:
            return np.zeros(n.shape)
        if kind == 1:
            d = R.bound(npairs, mag)
            dnum = (2 * np.abs(ref_image.real) + d) * d
            if np.iscomplexobj(ref_image):
                dnum = dnum + (2 * np.abs(ref_image.imag) + d) * d
            den = n * ref_sums[..., 1]
            F = factor_of(1, ref_image, ref_sums)
            return np.where(den > 0, dnum / (den * (1 - 2 * e)) + 2 * e * F + 8 * U * F, 0.0)
        d = e * n
        dnum = (2 * np.abs(ref_sums[..., 1]) + d) * d + (2 * np.abs(ref_sums[..., 2]) + d) * d
        return np.where(n > 0, np.sqrt(dnum / (n * n) + 8 * U) + 4 * U, 0.0)


def factor_ratio(kind, factor, ref_image, ref_sums, npairs, mag):
    """max |F - F_ref| / factor_bar (0 / 0 counts as 0; x / 0 as inf)."""
    err = np.abs(factor - factor_of(kind, ref_image, ref_sums))
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / factor_bar(kind, ref_image, ref_sums, npairs, mag))
    return float(np.nan_to_num(r, nan=np.inf).max())


# the demonstration: 8 elements, a point scatterer at node Q in complex Gaussian noise
DEMO_Q, DEMO_NT, DEMO_SIGMA = (25, 40), 700, 0.5


def demo_case(seed):
    """(T, fmc): the straight-ray fields of R.element_x(8, 6, 63) and the scatterer's echoes plus
    complex noise of standard deviation DEMO_SIGMA (DEMO_SIGMA / sqrt(2) per component)."""
    T = R.fields(R.element_x(8, 6, 63))
    tq = T[:, DEMO_Q[0], DEMO_Q[1]]
    fmc = R.scatterer_data(tq, tq, R.FS, DEMO_NT)
    g = np.random.default_rng(seed).standard_normal(fmc.shape + (2,)) * (DEMO_SIGMA / np.sqrt(2.0))
    return T, (fmc + (g[..., 0] + 1j * g[..., 1])).astype(np.complex64)


def demo_check(image, factor):
    """The demonstration's conditions on a plain image and its factor; returns (F at the
    scatterer, the largest F elsewhere, the gain of the peak-to-background ratio)."""
    q = DEMO_Q
    block = np.zeros(factor.shape, dtype=bool)
    block[q[0] - 2:q[0] + 3, q[1] - 2:q[1] + 3] = True
    plain, weighted = np.abs(image), np.abs(image * factor)
    assert np.unravel_index(weighted.argmax(), weighted.shape) == q
    f_in, f_out = float(factor[q]), float(factor[~block].max())
    gain = (weighted[q] / weighted[~block].max()) / (plain[q] / plain[~block].max())
    assert f_in >= 0.5 and f_out <= 0.2 and gain >= 4.0, (f_in, f_out, gain)
    return f_in, f_out, gain
