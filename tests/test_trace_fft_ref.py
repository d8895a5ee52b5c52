"""CPU checks of the spectral trace filter's contract (include/alifmm.h alifmm_trace_spectral): the
committed twiddle table against mpmath, the numpy restatement tests/trace_fft_ref.py against numpy's
FFT under the derived bar and against scipy's hilbert, and the kernel's own code
(csrc/trace_fft_term.h) run on the host under ASan and UBSan (tests/trace_fft_sim.cpp) against the
restatement, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import trace_fft_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ali-fmm-and-ray-tracing_amd", "csrc")


def test_table_is_mpmath_rounded_once():
    """All 2049 entries equal sin(2 pi m / 8192) at 300 bits rounded once, and the symmetries that
    serve the other quadrants and the cosines hold against mpmath too."""
    mpmath = pytest.importorskip("mpmath")
    tab = R.quarter_sines()
    assert tab.shape == (2049,) and tab[0] == 0.0 and not np.signbit(tab[0]) and tab[2048] == 1.0
    with mpmath.workprec(300):
        want = np.array([float(mpmath.sin(2 * mpmath.pi * m / 8192)) for m in range(2049)])
        assert np.array_equal(tab.view(np.uint64), want.view(np.uint64))
        m = np.arange(4096)
        c, s = R.twiddles(8192, m)
        for k in (0, 1, 1023, 2047, 2048, 2049, 3000, 4095):
            assert c[k] == float(mpmath.cos(2 * mpmath.pi * k / 8192)) or k == 2048
            assert s[k] == float(mpmath.sin(2 * mpmath.pi * k / 8192))
        assert c[2048] == 0.0  # cos(pi / 2) exactly, not its float64 neighbour
    # a smaller N reads the same numbers with a stride
    for n in (2, 8, 64, 4096):
        cn, sn = R.twiddles(n, np.arange(n // 2))
        assert np.array_equal(cn, c[::8192 // n]) and np.array_equal(sn, s[::8192 // n])
    assert np.array_equal(s[:2049], tab) and np.array_equal(s[2048:], tab[2048:0:-1])
    assert np.array_equal(c[:2049], tab[::-1]) and np.array_equal(c[2048:], -tab[:2048])


def test_shape_list():
    shapes = R.shapes()
    assert {s[2] for s in shapes} == {1 << k for k in range(14)}
    assert {s[1] for s in shapes} == {0} | {1 << k for k in range(14)}
    for n in (16, 8192):
        assert {s[0] for s in shapes if s[1] == n} == {1, n // 2 + 1, n - 1, n}


@pytest.mark.parametrize("name,cplx,f32,comp,analytic", R.TYPES)
def test_restatement_within_the_bar_of_numpy(name, cplx, f32, comp, analytic):
    """|restatement - np.fft route|_2 per trace under trace_fft_ref.bar on the whole shape list (the
    float64 values: the float32 rounding of the output is not part of the bar), and more than
    1e3 bars away with one twiddle of the forward transform zeroed."""
    worst = 0.0
    for nt, nfft, n in R.shapes():
        x, h = R.case(name, cplx, f32, comp, nt, n)
        got = R.restatement(x, h, analytic, nfft, round_out=False)
        want = R.exact_ref(x, h, analytic, nfft)
        b = R.bar(x, h, analytic, nfft)
        e = R.err2(got, want)
        assert got.shape == want.shape == x.shape and (e <= b).all(), (nt, nfft, (e / b).max())
        worst = max(worst, (e / b).max())
        if n >= 4 and nt == n:
            bad = R.restatement(x, h, analytic, nfft, round_out=False, zero_twiddle=(0, 1))
            assert (R.err2(bad, want) > 1e3 * b).all(), (nt, nfft)
    print("%s: worst |restatement - numpy| / bar = %.3g" % (name, worst))


def test_analytic_is_scipy_hilbert():
    signal = pytest.importorskip("scipy.signal")
    for n in (1, 2, 8, 256, 8192):
        x = R.noise((R.NTRACE, n), False, 50 + n)
        e = R.err2(R.restatement(x, None, True, n), signal.hilbert(x, N=n, axis=-1))
        assert (e <= R.bar(x, None, True, n)).all(), n
    # zero-padded: hilbert(x, N)[:nt]
    x = R.noise((R.NTRACE, 100), False, 51)
    e = R.err2(R.restatement(x, None, True, 128), signal.hilbert(x, N=128, axis=-1)[:, :100])
    assert (e <= R.bar(x, None, True, 128)).all()


def test_real_even_response_keeps_real_data_real():
    """A real H with H_k = H_{N-k} is a real filter: the imaginary part is rounding, under the bar."""
    for n in (8, 1024, 8192):
        h = R.noise(n, False, 60 + n)
        h[n // 2 + 1:] = h[1:n // 2][::-1]
        x = R.noise((R.NTRACE, n - 3), False, 61 + n)
        y = R.restatement(x, h, False, n)
        b = R.bar(x, h, False, n)
        assert (np.sqrt(np.sum(y.imag ** 2, axis=-1)) <= b).all() and (np.sqrt(np.sum(y.real ** 2, axis=-1)) > 1e6 * b).all()


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    d = tmp_path_factory.mktemp("trace_fft_sim")
    exe = str(d / "trace_fft_sim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(HERE, "trace_fft_sim.cpp"), "-o", exe],
                   check=True)

    def run(name, data, response, analytic, nfft):
        fin, fout = str(d / (name + ".in")), str(d / (name + ".out"))
        R.write_sim_input(fin, data, response, analytic, nfft)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        return R.read_sim_output(fout, data)

    return run


@pytest.mark.parametrize("name,cplx,f32,comp,analytic", R.TYPES)
def test_kernel_code_on_host_equals_the_restatement(sim, name, cplx, f32, comp, analytic):
    """The kernel's passes (every N from 1 to 8192: one pass without LDS up to 8 points, then every
    remainder of the first pass and two to five passes) give the restatement's bits."""
    for nt, nfft, n in R.shapes():
        x, h = R.case(name, cplx, f32, comp, nt, n)
        got = sim(name, x, h, analytic, nfft)
        want = R.restatement(x, h, analytic, nfft)
        assert got.dtype == want.dtype and np.array_equal(got, want), (nt, nfft)
        assert want.any()


def test_kernel_code_on_host_many_traces(sim):
    """More traces than a workgroup packs, and not a multiple of it: every trace is reached, and a
    trace alone has the bits it has among the others."""
    x = R.noise((67, 100), False, 71, f32=True)
    want = R.restatement(x, None, True, 128)
    assert np.array_equal(sim("many", x, None, True, 128), want)
    for k in (0, 16, 66):
        assert np.array_equal(R.restatement(x[k], None, True, 128), want[k])


def test_bandpass_response():
    """Host numpy: flat inside the band, raised-cosine edges, even in frequency, edges checked."""
    import _alifmm

    n, fs = 256, 50e6
    h = _alifmm.bandpass_response(n, fs, 3e6, 7e6, 1e6)
    f = np.abs(np.fft.fftfreq(n, 1 / fs))
    assert h.shape == (n,) and h.dtype == np.float64 and h.min() == 0.0 and h.max() == 1.0
    assert (h[(f >= 3e6) & (f <= 7e6)] == 1.0).all() and (h[(f <= 2e6) | (f >= 8e6)] == 0.0).all()
    edge = (f > 2e6) & (f < 3e6)
    assert edge.any() and ((h[edge] > 0) & (h[edge] < 1)).all()
    assert np.array_equal(h[1:], h[1:][::-1])  # H_k = H_{N-k}
    assert np.array_equal(_alifmm.bandpass_response(n, fs, 3e6, 7e6, 0.0), ((f >= 3e6) & (f <= 7e6)).astype(float))
    for lo, hi in ((-1.0, 5e6), (5e6, 5e6), (7e6, 3e6), (3e6, 26e6), (np.nan, 5e6)):
        with pytest.raises(ValueError, match="band edges"):
            _alifmm.bandpass_response(n, fs, lo, hi)
    with pytest.raises(ValueError):
        _alifmm.bandpass_response(n, fs, 3e6, 7e6, -1.0)
