"""CPU checks of the trace FIR contract (include/alifmm.h alifmm_trace_fir): the numpy restatement
tests/trace_fir_ref.py against itself (the transposed sum is the transpose of the forward one, to
the bit) and against numpy's convolution, and the kernel's own code (csrc/trace_fir_term.h) run on
the host under ASan and UBSan (tests/trace_fir_sim.cpp) against the restatement, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import trace_fir_ref as F

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ali-fmm-and-ray-tracing_amd", "csrc")
SIM_TILE = 64  # the program's tile: the shape list of the GPU test with the kernel's tile replaced by it


@pytest.mark.parametrize("name,cplx_data,cplx_taps", F.TYPES)
def test_transposed_restatement_is_the_transpose(name, cplx_data, cplx_taps):
    """The dense real matrix of the transposed sum equals the transpose of the forward one exactly:
    an entry is one tap (or its negation), set by one product with 1.0 and one add to 0.0."""
    ncomp = 2 if cplx_data else 1
    for nt, ntap, origin in ((9, 1, 0), (9, 4, 0), (9, 4, 3), (9, 5, 2), (5, 17, 8), (12, 17, 0), (12, 17, 16)):
        h = F.noise_taps(ntap, cplx_taps)
        P = F.dense_P(nt, h, origin, ncomp)
        Pt = F.dense_P(nt, h, origin, ncomp, transpose=True)
        assert P.any() and np.array_equal(Pt, P.T), (nt, ntap, origin)
        # and the matrix is the operator: P x by the matrix, to rounding
        x = F.noise((nt,), cplx_data, 5)
        y = F.fir_ref(x, h, origin)
        assert np.allclose(P @ F.interleave(x), F.interleave(y), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("name,cplx_data,cplx_taps", F.TYPES)
def test_origin_zero_is_the_causal_convolution(name, cplx_data, cplx_taps):
    """origin = 0 is np.convolve(x, h)[:nt], the convention of ALI_FMM.simulate_fmc, to rounding;
    another origin shifts the same full convolution."""
    for nt, ntap in ((40, 1), (40, 7), (40, 33), (10, 33)):
        h = F.pulse(ntap, 3, cplx_taps) if ntap > 1 else np.array([0.75 - 0.5j]) if cplx_taps else np.array([0.75])
        x = F.noise((3, nt), cplx_data, 9)
        full = np.stack([np.convolve(t, h) for t in x])
        scale = np.abs(full).max()
        assert np.abs(F.fir_ref(x, h, 0) - full[:, :nt]).max() <= 1e-14 * scale
        for origin in (ntap // 2, ntap - 1):
            assert np.abs(F.fir_ref(x, h, origin) - full[:, origin:origin + nt]).max() <= 1e-14 * scale


def test_a_sample_outside_the_trace_adds_nothing():
    """A non-finite sample reaches exactly the outputs whose sums read it."""
    nt, ntap, origin = 20, 5, 1
    x = F.noise((nt,), False, 2)
    x[7] = np.inf
    y = F.fir_ref(x, np.ones(ntap), origin)
    assert np.array_equal(~np.isfinite(y), (np.arange(nt) >= 7 - origin) & (np.arange(nt) <= 7 - origin + ntap - 1))
    z = F.fir_ref(x, np.ones(ntap), origin, transpose=True)
    assert np.array_equal(~np.isfinite(z), (np.arange(nt) >= 7 + origin - ntap + 1) & (np.arange(nt) <= 7 + origin))


def test_adjoint_bar_holds_for_the_restatement(capsys):
    for name, cplx_data, cplx_taps in F.TYPES:
        h = F.pulse(33, 5, cplx_taps)
        x, y = F.noise((3, 200), cplx_data, 11), F.noise((3, 200), cplx_data, 12)
        lhs, rhs = F.real_dot(F.fir_ref(x, h, 16), y), F.real_dot(x, F.fir_ref(y, h, 16, transpose=True))
        bar, S = F.adjoint_bar(x, y, h, 16)
        print("%s: |<Px, y> - <x, P^T y>| / bar = %.3g" % (name, abs(lhs - rhs) / bar))
        assert abs(lhs - rhs) <= bar and abs(lhs) > 1e3 * bar
        # a dropped tap is far outside it
        h2 = h.copy()
        h2[20] = 0
        assert abs(F.real_dot(F.fir_ref(x, h2, 16), y) - rhs) > 1e3 * bar


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    d = tmp_path_factory.mktemp("trace_fir_sim")
    exe = str(d / "trace_fir_sim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(HERE, "trace_fir_sim.cpp"), "-o", exe],
                   check=True)

    def run(name, data, taps, origin, transpose, tile=SIM_TILE):
        fin, fout = str(d / (name + ".in")), str(d / (name + ".out"))
        F.write_sim_input(fin, data, taps, origin, transpose, tile)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        return F.read_sim_output(fout, data)

    return run


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("name,cplx_data,cplx_taps", F.TYPES)
def test_kernel_code_on_host_equals_the_restatement(sim, name, cplx_data, cplx_taps, transpose):
    """The tiled walk of the kernel (tile 64) gives the restatement's bits on every shape of the GPU
    test's list: traces shorter than a tile and than the pulse, tile edges, a halo longer than a
    tile (69 and 1024 taps), the cap, every origin."""
    shapes = F.shapes(SIM_TILE)
    assert len(shapes) == 72
    for nt, ntap, origin in shapes:
        x = F.noise((3, nt), cplx_data, 100 + nt)
        h = F.noise_taps(ntap, cplx_taps)
        got = sim("%s_%d" % (name, transpose), x, h, origin, transpose)
        want = F.fir_ref(x, h, origin, transpose)
        assert got.dtype == want.dtype and np.array_equal(got, want), (nt, ntap, origin)
        assert want.any()


def test_kernel_code_on_host_other_tiles_and_many_traces(sim):
    """The result does not depend on the tile (4, the smallest, to 1024, the kernel's), and the
    trace index reaches every trace."""
    x = F.noise((67, 150), True, 21)
    h = F.pulse(17, 3, True)
    want = F.fir_ref(x, h, 8)
    for tile in (4, 8, 128, 1024):
        assert np.array_equal(sim("tiles", x, h, 8, False, tile), want), tile
    want_t = F.fir_ref(x, h, 8, True)
    assert np.array_equal(sim("tiles", x, h, 8, True, 1024), want_t) and not np.array_equal(want, want_t)
    for k in (0, 33, 66):
        assert np.array_equal(want[k], F.fir_ref(x[k], h, 8))
