"""CPU checks of the coherence-weighted TFM contract (include/alifmm.h alifmm_tfm_coh): the numpy
reference tests/tfm_coh_ref.py against a scalar loop and against tfm_ref.py's image, the kernel's own
per-pixel code (csrc/tfm_coh_term.h) run on the host under UBSan (tests/tfm_coh_sim.cpp) against the
reference and, to the bit, against tfm_sim's image, and the demonstration case of the GPU tests.

The bars are tfm_coh_ref.py's (derived there): n and b exact, |q - q_ref| <= 2 (npairs + 4) 2^-53
q_ref, |ph_c - ph_c,ref| <= 2 (npairs + 4) 2^-53 n, the factor bit-equal to the formula on the
program's own image and sums, and within factor_bar() of the reference's."""
import math
import os
import subprocess

import numpy as np
import pytest

import tfm_coh_ref as C
import tfm_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ali-fmm-and-ray-tracing_amd", "csrc")
KINDS = {1: (1, 2), 2: (1, 2, 3)}  # by ncomp


def _scalar(ttx, trx, s, fs, t0, w, kind):
    ntx, nrx, nt, nc = s.shape
    niz, nix = ttx.shape[1:]
    img, sums, fac = np.zeros((niz, nix, nc)), np.zeros((niz, nix, 3)), np.zeros((niz, nix))
    for i in range(niz):
        for j in range(nix):
            S, n, x = [0.0] * nc, 0.0, [0.0, 0.0]
            for a in range(ntx):
                for b in range(nrx):
                    wt = 1.0 if w is None else float(w[a, b])
                    u = ((float(ttx[a, i, j]) + float(trx[b, i, j])) - t0) * fs
                    if wt == 0.0 or not (u >= 0.0 and u < nt - 1):
                        continue
                    k = int(u)
                    f = u - float(k)
                    t = [wt * (float(s[a, b, k, c]) + f * (float(s[a, b, k + 1, c]) - float(s[a, b, k, c]))) for c in range(nc)]
                    for c in range(nc):
                        S[c] += t[c]
                    n += 1.0
                    e = t[0] * t[0]
                    if nc == 2:
                        e = e + t[1] * t[1]
                    if kind == 1:
                        x[0] += e
                    elif kind == 2:
                        x[0] += (t[0] > 0) - (t[0] < 0)
                    else:
                        g = math.sqrt(e)
                        if g > 0:
                            r = 1.0 / g
                            x[0] += t[0] * r
                            x[1] += t[1] * r
            img[i, j], sums[i, j] = S, (n, x[0], x[1])
            if kind == 1:
                num = S[0] * S[0]
                if nc == 2:
                    num = num + S[1] * S[1]
                fac[i, j] = num / (n * x[0]) if n * x[0] > 0 else 0.0
            elif n > 0:
                if kind == 2:
                    m = x[0] / n
                    y = 1.0 - m * m
                else:
                    y = max(1.0 - (x[0] * x[0] + x[1] * x[1]) / (n * n), 0.0)
                fac[i, j] = 1.0 - math.sqrt(y)
    return img, fac, sums


@pytest.mark.parametrize("ncomp", [1, 2])
def test_reference_equals_scalar_loop(ncomp):
    rng = np.random.default_rng(11)
    nt, fs, t0 = 9, 2.0, 0.5
    ttx = rng.uniform(0.0, 2.6, (3, 5, 6))
    trx = rng.uniform(0.0, 2.6, (2, 5, 6))
    ttx[0, 1, 2], trx[1, 3, 3], ttx[2, 4, 5] = np.nan, np.inf, -3.0
    fmc = R.data(3, 2, nt=nt, ncomp=ncomp, seed=3).copy()
    fmc[2, 1] = 0  # counting terms of value 0
    w = np.array([[1.0, 0.0], [0.5, -2.0], [1.5, 1.0]], dtype=np.float32)
    for wt in (None, w):
        plain, pmag, cnt = R.tfm_ref(ttx, trx, fmc, fs, t0, wt)
        for kind in KINDS[ncomp]:
            img, fac, sums, mag = C.tfm_coh_ref(ttx, trx, fmc, fs, kind, t0, wt)
            # same pair order (a, then b) and the same operations: the same bits
            assert np.array_equal(img, plain) and np.array_equal(mag, pmag)
            si, sf, ss = _scalar(ttx, trx, R.as_samples(fmc), fs, t0, wt, kind)
            si = si.view(np.complex128)[..., 0] if ncomp == 2 else si[..., 0]
            assert np.array_equal(img, si) and np.array_equal(sums, ss) and np.array_equal(fac, sf)
            assert sums[..., 0].sum() == cnt["inside"]
            assert np.all((fac >= 0) & (fac <= 1 + 1e-15))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    d = tmp_path_factory.mktemp("tfm_coh_sim")
    exes = {}
    for name in ("tfm_sim", "tfm_coh_sim"):
        exes[name] = str(d / name)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=undefined,float-cast-overflow",
                        "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(HERE, name + ".cpp"), "-o", exes[name]],
                       check=True)

    def run(name, flds, tx, rx, fmc, fs, t0, w, window, step, kind, chunk=8):
        """(image, factor, sums) of tfm_coh_sim, and tfm_sim's image on the same input file."""
        fin = str(d / (name + ".in"))
        R.write_sim_input(fin, flds, tx, rx, fmc, fs, t0, w, window, step)
        nc = 2 if np.iscomplexobj(fmc) else 1
        npix = window[2] * window[3]
        outs = []
        for exe, extra in (("tfm_coh_sim", [str(kind), str(chunk)]), ("tfm_sim", [])):
            fout = str(d / (name + "." + exe))
            r = subprocess.run([exes[exe], fin, fout] + extra, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (exe, r.returncode, r.stdout, r.stderr)
            outs.append(np.fromfile(fout, dtype=np.float64))
        o, plain = outs
        assert o.size == npix * (nc + 4) and plain.size == npix * nc
        cx = lambda a: a.reshape(window[2], window[3], nc).view(np.complex128)[..., 0] if nc == 2 else a.reshape(window[2:])
        return (cx(o[:npix * nc]), o[npix * nc:npix * (nc + 1)].reshape(window[2:]),
                o[npix * (nc + 1):].reshape(window[2], window[3], 3), cx(plain))

    return run


def _compare(kind, got, ref, npairs, chunk_default=True):
    img, fac, sums, plain = got
    rimg, rfac, rsums, mag = ref
    if chunk_default:
        assert np.array_equal(img, plain)  # tfm_term's sum, statement for statement
    assert R.worst_ratio(img, rimg, npairs, mag) <= 1.0
    assert C.sums_ratio(kind, sums, rsums, npairs) <= 1.0
    assert np.array_equal(fac, C.factor_of(kind, img, sums))
    assert C.factor_ratio(kind, fac, rimg, rsums, npairs, mag) <= 1.0
    none = rsums[..., 0] == 0  # no counting term
    assert np.all(img[none] == 0) and not sums[none].any() and not fac[none].any()


@pytest.mark.parametrize("ncomp", [1, 2])
def test_kernel_term_code_on_host_seven_elements(sim, ncomp):
    T = R.fields(R.element_x(7))
    fmc = R.data(7, 7, ncomp=ncomp)
    idx = list(range(7))
    for kind in KINDS[ncomp]:
        outs = {}
        for name, win, step in (("full", R.full_window(T.shape[1:]), 1), ("win", R.WINDOW, 1), ("s3", R.WINDOW_STEP3, 3)):
            got = sim("e7_%s_%d_%d" % (name, ncomp, kind), T, idx, idx, fmc, R.FS, R.T0, None, win, step, kind)
            _compare(kind, got, C.tfm_coh_ref(T, T, fmc, R.FS, kind, R.T0, None, win, step), 49)
            outs[name] = got[:3]
        # a pixel has the same bits through every window and step
        for name, (a, b, c, d), st in (("win", R.WINDOW, 1), ("s3", R.WINDOW_STEP3, 3)):
            for x, full in zip(outs[name], outs["full"]):
                assert np.array_equal(x, full[a:a + st * c:st, b:b + st * d:st])


def test_kernel_term_code_on_host_chunks_weights_and_zero_terms(sim):
    """4 x 9 pairs (a partial last chunk for every chunk size), nt = 2, weights with zeros and
    negative values, slot lists that repeat, one transmitter's data all zero (counting terms of
    value 0: the phase sum skips them, n does not).  n and b do not depend on the chunk."""
    rng = np.random.default_rng(2)
    T = R.fields(R.element_x(9))
    tx, rx = [8, 3, 3, 1], [1, 2, 3, 4, 5, 6, 7, 0, 4]
    fmc = R.data(4, 9, nt=2).copy()
    fmc[1] = 0
    w = rng.standard_normal((4, 9)).astype(np.float32)
    w[rng.random((4, 9)) < 0.3] = 0
    assert (w == 0).any() and (w < 0).any() and (w[1] != 0).any()
    win = R.full_window(T.shape[1:])
    fs, t0 = 1.2e5, 2e-6  # u spans about [-0.24, 3.3]
    for kind in (1, 2, 3):
        ref = C.tfm_coh_ref(T[tx], T[rx], fmc, fs, kind, t0, w, win, 1)
        base = None
        for chunk in (8, 4, 16, 32):
            got = sim("chunk%d_%d" % (chunk, kind), T, tx, rx, fmc, fs, t0, w, win, 1, kind, chunk)
            _compare(kind, got, ref, 36, chunk == 8)
            base = got if base is None else base
            assert np.array_equal(got[2][..., 0], base[2][..., 0])
            assert kind != 2 or np.array_equal(got[2], base[2])
    # the zero-valued terms count: without them n is smaller somewhere
    w0 = w.copy()
    w0[1] = 0
    less = C.tfm_coh_ref(T[tx], T[rx], fmc, fs, 3, t0, w0, win, 1)
    assert (less[2][..., 0] < ref[2][..., 0]).any() and np.array_equal(less[2][..., 1:], ref[2][..., 1:])


def test_kernel_term_code_on_host_edge_delays(sim):
    """The one-pixel cases of test_tfm_ref.py's edge-delay row: -0.0, nt - 1 and one ulp below it,
    NaN, +-inf, 2^31, 2^63 ...  A second transmitter of NaN delays carries weight 0.  Terms that do
    not count leave every sum untouched: image, factor and sums are exactly 0 there; UBSan
    (float-cast-overflow) aborts the program if one of them reaches the integer conversion.  A
    pixel with its one term has n = 1, and its factor is 1 (CF, SCF: exactly)."""
    nt = 12
    edge = np.array([0.0, nt - 1.0, math.nextafter(nt - 1.0, 0.0), -0.0, -1.5, np.nan, np.inf, -np.inf, 1e300,
                     3.25, 2.0 ** 31, 2.0 ** 63, -2.0 ** 63, 5e-324, 10.999])
    inside = np.array([1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1], dtype=bool)
    n = len(edge)
    win = (0, 0, 1, n)
    flds = np.stack([edge[None, :], np.full((1, n), -0.0), np.full((1, n), np.nan)])
    for ncomp in (1, 2):
        fmc = R.data(2, 1, nt=nt, ncomp=ncomp)
        for kind in KINDS[ncomp]:
            for w in (np.array([[1.0], [0.0]], dtype=np.float32), np.array([[-0.75], [0.0]], dtype=np.float32), None):
                got = sim("edge", flds, [0, 2], [1], fmc, 1.0, 0.0, w, win, 1, kind)
                _compare(kind, got, C.tfm_coh_ref(flds[[0, 2]], flds[[1]], fmc, 1.0, kind, 0.0, w, win, 1), 2)
                img, fac, sums, _ = got
                assert np.array_equal(sums[0, :, 0], inside.astype(float))
                assert np.all(img[0, ~inside] == 0) and not fac[0, ~inside].any() and not sums[0, ~inside].any()
                assert np.all(img[0, inside] != 0)
                if kind == 3:
                    assert np.all(np.abs(fac[0, inside] - 1) <= 1e-7)
                    assert np.all(np.abs(np.hypot(sums[0, inside, 1], sums[0, inside, 2]) - 1) <= 4 * C.U)
                else:
                    assert np.all(fac[0, inside] == 1)
                if kind == 2:
                    assert np.array_equal(sums[0, inside, 1], np.sign(img.real[0, inside]))


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_demonstration_case_meets_its_conditions(seed):
    """The inputs of the GPU demonstration, in the reference alone: every kind's weighted image
    peaks at the scatterer, F >= 0.5 there and <= 0.2 outside the 5 x 5 block around it, and the
    peak-to-background ratio gains at least 4 x over the plain image."""
    T, fmc = C.demo_case(seed)
    for kind in ("cf", "scf", "pcf"):
        img, fac, _, _ = C.tfm_coh_ref(T, T, fmc, R.FS, kind)
        f_in, f_out, gain = C.demo_check(img, fac)
        print("seed %d %s: F %.3f at the scatterer, <= %.3f elsewhere, ratio gain %.1f x" % (seed, kind, f_in, f_out, gain))
