"""CPU checks of the least-squares imaging contract (include/alifmm.h alifmm_tfm_f64, alifmm_tfm_lsq):
the numpy restatement tests/tfm_lsq_ref.py against numpy's lstsq and against itself (Aᵀ as a matrix
and as the delay-and-sum), the conditioning of the solve cases the GPU tests use, and the solve's
own code (csrc/tfm_term.h in float64, csrc/tfm_model_term.h, csrc/tfm_solve_ops.h, csrc/solve_ops.h)
run on the host under ASan and UBSan (tests/tfm_lsq_sim.cpp)."""
import math
import os
import subprocess

import numpy as np
import pytest

import tfm_lsq_ref as L
import tfm_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ali-fmm-and-ray-tracing_amd", "csrc")

# name -> (rows, columns, sigma_max, sigma_min, rank) of the operator
TABLE = {"e7": (23520, 117, 10.1, 4.15, 117), "e7s3": (23520, 200, 8.94, 3.99, 200), "e2": (1920, 117, 3.29, 0.47, 117),
         "e1": (480, 117, 1.62, 0.0, 106)}
# iterations of the restatement at tol 1e-10 without smoothing, complex data
ITERS = {"e7": 21, "e7s3": 19, "e2": 61, "e1": 121}


@pytest.mark.parametrize("name", list(L.CASES))
def test_operator_cases(name):
    c = L.case(name)
    rows, cols, smax, smin, rank = TABLE[name]
    sv = c["sv"]
    print("%s: A %s, sigma %.4g .. %.4g, rank %d" % (name, c["A"].shape, sv[0], sv[-1], np.linalg.matrix_rank(c["A"])))
    assert c["A"].shape == (rows, cols)
    assert abs(sv[0] - smax) <= 0.006 * smax and abs(sv[-1] - smin) <= 0.01
    assert np.linalg.matrix_rank(c["A"]) == rank


@pytest.mark.parametrize("ncomp", [1, 2])
@pytest.mark.parametrize("name", list(L.CASES))
def test_adjoint_matrix_equals_delay_and_sum(name, ncomp):
    """Aᵀ d by the dense matrix against the float64 delay-and-sum restatement, within tfm_ref.bound
    (the matrix holds 1 - f and f, the sum interpolates: other roundings of the same magnitude)."""
    c = L.case(name)
    d = L.noise64(c["n"], c["n"], ncomp=ncomp)
    img, mag = L.tfm_f64_ref(c["T"], c["T"], d, R.FS, R.T0, None, c["window"], c["step"])
    at = L.from_columns(c["A"].T @ L.columns(d), img.shape)
    r = R.worst_ratio(at, img, c["n"] ** 2, mag)
    print("%s c%d: worst |A^T d - tfm_f64(d)| / bound = %.3g" % (name, ncomp, r))
    assert r <= 1.0
    # and the float32 cast of the data is another image altogether
    img32, _ = L.tfm_f64_ref(c["T"], c["T"], d.astype(np.complex64 if ncomp == 2 else np.float32), R.FS, R.T0, None,
                             c["window"], c["step"])
    r32 = R.worst_ratio(img32, img, c["n"] ** 2, mag)
    print("%s c%d: the float32 cast misses the bar by %.3g (asked: %.3g)" % (name, ncomp, r32, L.cast_gap(c["n"] ** 2)))
    assert r32 > L.cast_gap(c["n"] ** 2)


def test_f64_restatement_equals_f32_restatement_on_f32_data():
    T = R.fields(R.element_x(7))
    for ncomp in (1, 2):
        d = R.data(7, 7, ncomp=ncomp)
        a, mag, _ = R.tfm_ref(T, T, d, R.FS, R.T0, None, R.WINDOW)
        b, mag64 = L.tfm_f64_ref(T, T, d.astype(np.complex128 if ncomp == 2 else np.float64), R.FS, R.T0, None, R.WINDOW)
        assert np.array_equal(a, b) and np.array_equal(mag, mag64)


@pytest.mark.parametrize("smooth_on", [False, True])
@pytest.mark.parametrize("ncomp", [1, 2])
@pytest.mark.parametrize("name", list(L.CASES))
def test_cgls_against_lstsq(name, ncomp, smooth_on):
    """The restatement stops by tol and lies as close to numpy's lstsq on the stacked system as its
    gradient allows: |x - x*| <= |Bᵀ(b - B x)| / sigma_min(B)², the true gradient being at most
    2 tol |Bᵀ b|.  At the stop gamma is not within 1e-6 of the threshold, nor one iteration earlier,
    so an iteration count can be compared across summation orders."""
    c, rhs, damp, smooth = L.problem(name, ncomp, smooth_on)
    B, _ = L.stacked(c["A"], c["D"], rhs, damp, smooth)
    smin = np.linalg.svd(B, compute_uv=False)[-1]
    xl = L.lstsq(c["A"], c["D"], rhs, damp, smooth)
    for tol in (1e-8, 1e-10):
        x, info, r = L.cgls(c["A"], c["D"], rhs, damp, smooth, 400, tol)
        g, g0 = L.true_gradient(c["A"], c["D"], rhs, damp, smooth, x)
        dev = L.deviation(x, xl)
        thr = tol * tol * info["gammas"][0]
        last, prev = info["gammas"][-1] / thr, info["gammas"][-2] / thr
        print("%s c%d smooth %d tol %g: %d iterations, deviation %.3g, gradient %.3g of %.3g, gamma / threshold %.3g "
              "(%.3g before)" % (name, ncomp, smooth_on, tol, info["iterations"], dev, g, g0, last, prev))
        assert info["reason"] == "tol"
        assert g <= 2 * tol * g0
        assert dev <= g / (smin * smin * np.linalg.norm(xl)) + 1e-13
        assert abs(last - 1) > 1e-6 and abs(prev - 1) > 1e-6
        assert abs(info["grad0"] - g0) <= 1e-12 * g0
        assert abs(info["res_norm"] - np.linalg.norm(rhs - c["A"] @ x)) <= 1e-10 * info["rhs_norm"]
        if tol == 1e-10 and ncomp == 2 and not smooth_on:
            assert info["iterations"] == ITERS[name]


def test_difference_is_the_stencil():
    niz, nix = 5, 7
    D = L.difference(niz, nix)
    v = np.random.default_rng(1).standard_normal((niz, nix))
    ref = np.zeros((niz, nix))
    for z in range(niz):
        for x in range(nix):
            for zz, xx in ((z - 1, x), (z, x - 1), (z, x + 1), (z + 1, x)):
                if 0 <= zz < niz and 0 <= xx < nix:
                    ref[z, x] += v[z, x] - v[zz, xx]
    assert np.allclose((D.T @ D @ v.ravel()).reshape(niz, nix), ref, rtol=0, atol=1e-13)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    d = tmp_path_factory.mktemp("tfm_lsq_sim")
    exe = str(d / "tfm_lsq_sim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(HERE, "tfm_lsq_sim.cpp"), "-o", exe],
                   check=True)

    def run(name, flds, tx, rx, fmc, fs, t0, w, window, step, damp=0.0, smooth=0.0, max_iter=1, tol=0.0):
        fin, fout = str(d / (name + ".in")), str(d / (name + ".out"))
        L.write_sim_input(fin, flds, tx, rx, fmc, fs, t0, w, window, step, damp, smooth, max_iter, tol)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        nc = 2 if np.iscomplexobj(fmc) else 1
        ni, nd = window[2] * window[3] * nc, np.asarray(fmc).size * nc
        atd, x, res, info = L.read_sim_output(fout, ni, nd)
        shape = (window[2], window[3])
        return (L.from_columns(atd.reshape(-1, nc), shape), L.from_columns(x.reshape(-1, nc), shape),
                L.from_columns(res.reshape(-1, nc), np.shape(fmc)), info)

    return run


def test_f64_term_code_on_host_edge_delays(sim):
    """test_tfm_ref.py's edge-delay table through the float64 instantiation of tfm_term.h: the
    transmitter field holds the edge delays, the receiver field -0.0, fs = 1 and t0 = 0, so u is the
    table entry itself; a second transmitter of NaN delays carries weight 0.  Out-of-range,
    non-finite and zero-weight entries are exactly 0; UBSan aborts the program if one of them
    reaches the integer conversion."""
    nt = 12
    edge = np.array([0.0, nt - 1.0, math.nextafter(nt - 1.0, 0.0), -0.0, -1.5, np.nan, np.inf, -np.inf, 1e300,
                     3.25, 2.0 ** 31, 2.0 ** 63, -2.0 ** 63, 5e-324, 10.999])
    inside = np.array([1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1], dtype=bool)
    n = len(edge)
    flds = np.stack([edge[None, :], np.full((1, n), -0.0), np.full((1, n), np.nan)])
    fmc = L.noise64(2, 1, nt=nt)
    for w in (np.array([[1.0], [0.0]], dtype=np.float32), np.array([[-0.75], [0.0]], dtype=np.float32)):
        img = sim("edge", flds, [0, 2], [1], fmc, 1.0, 0.0, w, (0, 0, 1, n), 1)[0]
        ref, mag = L.tfm_f64_ref(flds[[0, 2]], flds[[1]], fmc, 1.0, 0.0, w, (0, 0, 1, n), 1)
        assert np.array_equal(mag[0] > 0, inside)
        assert np.all(img[0, ~inside] == 0) and np.all(img[0, inside] != 0)
        assert R.worst_ratio(img, ref, 2, mag) <= 1.0
    assert img[0, 3] == -0.75 * fmc[0, 0, 0] and img[0, 0] == -0.75 * fmc[0, 0, 0]  # float64 samples, unrounded


@pytest.mark.parametrize("ncomp", [1, 2])
def test_f64_term_code_on_host_bits_of_f32(sim, ncomp):
    """On float32-representable data the float64 instantiation gives the bits of the float32
    restatement (whose pair order a, then b is the chunk order for nrx <= 8)."""
    T = R.fields(R.element_x(7))
    d32 = R.data(7, 7, ncomp=ncomp)
    idx = list(range(7))
    img = sim("bits%d" % ncomp, T, idx, idx, d32.astype(np.complex128 if ncomp == 2 else np.float64), R.FS, R.T0, None,
              R.WINDOW, 1)[0]
    ref, _, _ = R.tfm_ref(T, T, d32, R.FS, R.T0, None, R.WINDOW)
    assert np.array_equal(img, ref)


@pytest.mark.parametrize("name,ncomp,smooth_on", [("e7s3", 2, True), ("e2", 1, False), ("e1", 2, True)])
def test_solve_code_on_host(sim, name, ncomp, smooth_on):
    """The replay of alifmm_tfm_lsq against the restatement: Aᵀ d within tfm_ref.bound, the solve at
    tol 1e-10 within 8 e_ref of lstsq (e_ref the restatement's own deviation; the margin
    test_gpu_sens_solve.py grants another summation order), iterations within 1, the norms to 1e-9."""
    c, rhs, damp, smooth = L.problem(name, ncomp, smooth_on)
    d = L.data_of(c, rhs)
    idx = list(range(c["n"]))
    xr, ir, rr = L.cgls(c["A"], c["D"], rhs, damp, smooth, 400, 1e-10)
    xl = L.lstsq(c["A"], c["D"], rhs, damp, smooth)
    e_ref = L.deviation(xr, xl)
    atd, x, res, info = sim("%s_%d" % (name, ncomp), c["T"], idx, idx, d, R.FS, R.T0, None, c["window"], c["step"], damp,
                            smooth, 400, 1e-10)
    img, mag = L.tfm_f64_ref(c["T"], c["T"], d, R.FS, R.T0, None, c["window"], c["step"])
    assert R.worst_ratio(atd, img, c["n"] ** 2, mag) <= 1.0
    dev = L.deviation(L.columns(x), xl)
    print("%s c%d: host replay %d iterations (restatement %d), deviation %.3g, e_ref %.3g" %
          (name, ncomp, info[0], ir["iterations"], dev, e_ref))
    assert info[5] == 0 and abs(info[0] - ir["iterations"]) <= 1
    assert dev <= 8 * e_ref
    for k, key in ((1, "grad0"), (3, "rhs_norm"), (4, "res_norm")):
        assert abs(info[k] - ir[key]) <= 1e-9 * ir[key], key
    assert np.linalg.norm(L.columns(res) - (rhs - c["A"] @ L.columns(x))) <= 1e-12 * ir["rhs_norm"] * math.sqrt(rhs.size)
    # the first iterate, as max_iter = 1 gives it
    x1 = sim("%s_%d_one" % (name, ncomp), c["T"], idx, idx, d, R.FS, R.T0, None, c["window"], c["step"], damp, smooth, 1,
             0.0)
    xr1 = L.cgls(c["A"], c["D"], rhs, damp, smooth, 1, 0.0)[0]
    assert x1[3][0] == 1 and x1[3][5] == 1
    assert np.allclose(L.columns(x1[1]), xr1, rtol=1e-11, atol=1e-11 * np.abs(xr1).max())
