"""CPU checks of the TFM contract (include/alifmm.h alifmm_tfm): the numpy reference tests/tfm_ref.py
against a scalar loop, the coverage of the synthetic inputs the GPU tests use, window and step
independence, a point-scatterer image, and the kernel's own per-pixel code (csrc/tfm_term.h) run
on the host under UBSan (tests/tfm_sim.cpp)."""
import math
import os
import subprocess

import numpy as np
import pytest

import tfm_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ali-fmm-and-ray-tracing_amd", "csrc")


def _scalar(ttx, trx, s, fs, t0, w):
    ntx, nrx, nt, nc = s.shape
    niz, nix = ttx.shape[1:]
    img = np.zeros((niz, nix, nc))
    for i in range(niz):
        for j in range(nix):
            for a in range(ntx):
                for b in range(nrx):
                    wt = 1.0 if w is None else float(w[a, b])
                    if wt == 0.0:
                        continue
                    u = ((float(ttx[a, i, j]) + float(trx[b, i, j])) - t0) * fs
                    if not (u >= 0.0 and u < nt - 1):
                        continue
                    k = int(u)
                    f = u - float(k)
                    for c in range(nc):
                        x0, x1 = float(s[a, b, k, c]), float(s[a, b, k + 1, c])
                        img[i, j, c] += wt * (x0 + f * (x1 - x0))
    return img


@pytest.mark.parametrize("ncomp", [1, 2])
def test_reference_equals_scalar_loop(ncomp):
    rng = np.random.default_rng(11)
    nt, fs, t0 = 9, 2.0, 0.5
    ttx = rng.uniform(0.0, 2.6, (3, 5, 6))
    trx = rng.uniform(0.0, 2.6, (2, 5, 6))
    ttx[0, 1, 2], trx[1, 3, 3], ttx[2, 4, 5] = np.nan, np.inf, -3.0
    fmc = R.data(3, 2, nt=nt, ncomp=ncomp, seed=3)
    w = np.array([[1.0, 0.0], [0.5, -2.0], [1.5, 1.0]], dtype=np.float32)
    for wt in (None, w):
        img, mag, cnt = R.tfm_ref(ttx, trx, fmc, fs, t0, wt)
        ref = _scalar(ttx, trx, R.as_samples(fmc), fs, t0, wt)
        ref = ref.view(np.complex128)[..., 0] if ncomp == 2 else ref[..., 0]
        # same pair order (a, then b) and the same operations: the same bits
        assert np.array_equal(img, ref)
        assert sum(cnt.values()) == 3 * 2 * 30 and cnt["inside"] > 0 and cnt["nonfinite"] > 0
        assert cnt["below"] > 0 and cnt["above"] > 0 and (wt is None) == (cnt["zero_weight"] == 0)
        assert np.all(mag >= np.maximum(np.abs(img.real), np.abs(img.imag)) * (1 - 1e-12))


@pytest.mark.parametrize("n", [7, 65])
def test_synthetic_inputs_cover_the_range_test(n):
    """The inputs of the GPU tests exercise the range test on both sides: >= 90 % of the terms in
    range, >= 0.3 % below and >= 0.3 % above."""
    T = R.fields(R.element_x(n))
    _, _, cnt = R.tfm_ref(T, T, R.data(n, n), R.FS, R.T0, None, R.WINDOW)
    tot = n * n * R.WINDOW[2] * R.WINDOW[3]
    assert sum(cnt.values()) == tot and cnt["nonfinite"] == 0 and cnt["zero_weight"] == 0
    print("n=%d inside %.2f%% below %.2f%% above %.2f%%"
          % (n, 100 * cnt["inside"] / tot, 100 * cnt["below"] / tot, 100 * cnt["above"] / tot))
    assert cnt["inside"] >= 0.90 * tot
    assert cnt["below"] >= 0.003 * tot
    assert cnt["above"] >= 0.003 * tot


def test_window_and_step_independence():
    T = R.fields(R.element_x(7))
    fmc = R.data(7, 7)
    full, _, _ = R.tfm_ref(T, T, fmc, R.FS, R.T0)
    a, b, c, d = R.WINDOW
    win, _, _ = R.tfm_ref(T, T, fmc, R.FS, R.T0, None, R.WINDOW, 1)
    assert np.array_equal(win, full[a:a + c, b:b + d])
    a, b, c, d = R.WINDOW_STEP3
    win, _, _ = R.tfm_ref(T, T, fmc, R.FS, R.T0, None, R.WINDOW_STEP3, 3)
    assert np.array_equal(win, full[a:a + 3 * c:3, b:b + 3 * d:3])


def test_point_scatterer_focuses():
    xs = R.element_x(8, 6, 63)
    T = R.fields(xs)
    q = (25, 40)
    tq = T[:, q[0], q[1]]
    fmc = R.scatterer_data(tq, tq, R.FS, 700)
    img, _, _ = R.tfm_ref(T, T, fmc, R.FS, 0.0)
    mag = np.abs(img)
    peak = np.unravel_index(mag.argmax(), mag.shape)
    assert peak == q and mag[q] >= 0.7 * 64, (peak, mag[q])
    out = mag.copy()
    out[q[0] - 1:q[0] + 2, q[1] - 1:q[1] + 2] = 0
    print("peak %.1f at %s, largest outside the 3 x 3: %.1f" % (mag[q], peak, out.max()))
    assert out.max() <= 0.5 * mag[q]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    d = tmp_path_factory.mktemp("tfm_sim")
    exe = str(d / "tfm_sim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(HERE, "tfm_sim.cpp"), "-o", exe],
                   check=True)

    def run(name, flds, tx, rx, fmc, fs, t0, w, window, step):
        fin, fout = str(d / (name + ".in")), str(d / (name + ".out"))
        R.write_sim_input(fin, flds, tx, rx, fmc, fs, t0, w, window, step)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        nc = 2 if np.iscomplexobj(fmc) else 1
        img = np.fromfile(fout, dtype=np.float64).reshape(window[2], window[3], nc)
        return img.view(np.complex128)[..., 0] if nc == 2 else img[..., 0]

    return run


@pytest.mark.parametrize("ncomp", [1, 2])
def test_kernel_term_code_on_host_seven_elements(sim, ncomp):
    T = R.fields(R.element_x(7))
    fmc = R.data(7, 7, ncomp=ncomp)
    idx = list(range(7))
    for name, win, step in (("full", R.full_window(T.shape[1:]), 1), ("win", R.WINDOW, 1), ("s3", R.WINDOW_STEP3, 3)):
        img = sim("e7_%s_%d" % (name, ncomp), T, idx, idx, fmc, R.FS, R.T0, None, win, step)
        ref, mag, _ = R.tfm_ref(T, T, fmc, R.FS, R.T0, None, win, step)
        assert R.worst_ratio(img, ref, 49, mag) <= 1.0
        assert np.all(img[mag == 0] == 0)


def test_kernel_term_code_on_host_nt2_and_slot_lists(sim):
    """4 x 8 pairs, nt = 2 (only u in [0, 1) is in range), weights with zeros, slot lists that
    repeat and do not start at 0."""
    rng = np.random.default_rng(2)
    T = R.fields(R.element_x(9))
    tx, rx = [8, 3, 3, 1], [1, 2, 3, 4, 5, 6, 7, 0]
    fmc = R.data(4, 8, nt=2)
    w = rng.standard_normal((4, 8)).astype(np.float32)
    w[rng.random((4, 8)) < 0.3] = 0
    win = R.full_window(T.shape[1:])
    fs, t0 = 1.2e5, 2e-6  # u spans about [-0.24, 3.3]
    img = sim("nt2", T, tx, rx, fmc, fs, t0, w, win, 1)
    ref, mag, cnt = R.tfm_ref(T[tx], T[rx], fmc, fs, t0, w, win, 1)
    assert cnt["inside"] > 0 and cnt["below"] > 0 and cnt["above"] > 0 and cnt["zero_weight"] > 0
    assert R.worst_ratio(img, ref, 32, mag) <= 1.0
    assert np.all(img[mag == 0] == 0)


def test_kernel_term_code_on_host_edge_delays(sim):
    """One row of one-pixel cases: the transmitter field holds the edge delays, the receiver field
    -0.0, fs = 1 and t0 = 0, so u is the table entry itself.  A second transmitter of NaN delays
    carries weight 0.  Out-of-range, non-finite and zero-weight entries are exactly 0; UBSan
    (float-cast-overflow) aborts the program if one of them reaches the integer conversion."""
    nt = 12
    edge = np.array([0.0, nt - 1.0, math.nextafter(nt - 1.0, 0.0), -0.0, -1.5, np.nan, np.inf, -np.inf, 1e300,
                     3.25, 2.0 ** 31, 2.0 ** 63, -2.0 ** 63, 5e-324, 10.999])
    inside = np.array([1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1], dtype=bool)
    n = len(edge)
    flds = np.stack([edge[None, :], np.full((1, n), -0.0), np.full((1, n), np.nan)])
    fmc = R.data(2, 1, nt=nt)
    for w in (np.array([[1.0], [0.0]], dtype=np.float32), np.array([[-0.75], [0.0]], dtype=np.float32)):
        img = sim("edge", flds, [0, 2], [1], fmc, 1.0, 0.0, w, (0, 0, 1, n), 1)
        ref, mag, cnt = R.tfm_ref(flds[[0, 2]], flds[[1]], fmc, 1.0, 0.0, w, (0, 0, 1, n), 1)
        assert cnt["inside"] == inside.sum() and cnt["zero_weight"] == n
        assert np.array_equal(mag[0] > 0, inside)
        assert np.all(img[0, ~inside] == 0) and np.all(img[0, inside] != 0)
        assert R.worst_ratio(img, ref, 2, mag) <= 1.0
    # u = -0.0 reads sample 0 exactly, u one ulp below nt - 1 interpolates the last two samples
    s = R.as_samples(fmc)[0, 0].astype(np.float64).view(np.complex128)[:, 0]
    assert img[0, 3] == -0.75 * s[0] and img[0, 0] == -0.75 * s[0]
    # without the zero weight the NaN transmitter is a term like any other: out of range, 0
    img = sim("edge1", flds, [0, 2], [1], fmc, 1.0, 0.0, None, (0, 0, 1, n), 1)
    assert np.all(img[0, ~inside] == 0) and np.all(img[0, inside] != 0)
