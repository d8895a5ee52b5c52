"""GPU tests of the spectral trace filter (include/alifmm.h alifmm_trace_spectral; csrc/trace_fft.hip,
the arithmetic of csrc/trace_fft_term.h) against the numpy restatement tests/trace_fft_ref.py.  The
contract fixes the order of every operation, so the comparisons are equalities of bits
(np.array_equal), not tolerances."""
import numpy as np
import pytest

import trace_fft_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)  # no model: the filter needs none
    yield c
    c.close()


# ---- 1. bit equality against the restatement ----

@pytest.mark.parametrize("name,cplx,f32,comp,analytic", R.TYPES)
def test_bits_against_the_restatement(ctx, name, cplx, f32, comp, analytic):
    """Seeded noise, 3 traces, every transform length from 1 to 8192 (a transform in registers up
    to 8 points, then every remainder of the first pass, two to five passes, several traces and one
    trace per workgroup, the LDS image beyond 64 KiB at 4096 and 8192); traces of 1, N / 2 + 1,
    N - 1 and N samples; the automatic length."""
    for nt, nfft, n in R.shapes():
        x, h = R.case(name, cplx, f32, comp, nt, n)
        got = ctx.trace_spectral(x, response=h, analytic=analytic, nfft=nfft)
        want = R.restatement(x, h, analytic, nfft)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert np.array_equal(got, want), (nt, nfft, np.abs(got - want).max())
        assert want.any()
    assert ctx.get_option("trace_fft_kernel_ms") > 0 and ctx.get_option("trace_fft_upload_ms") > 0


def test_bits_on_many_traces(ctx):
    """65 x 65 traces of 100 samples (N = 128: 16 traces per workgroup, the last workgroup holding
    one); 2 grid + 1 traces at N = 8; and 2 grid batches of traces and one more at N = 8, more
    batches than the launch has workgroups, so every workgroup walks its share with the grid's
    stride."""
    x = R.noise((65, 65, 100), False, 31, f32=True)
    got = ctx.trace_spectral(x, analytic=True, nfft=128)
    assert got.shape == x.shape and got.dtype == np.complex64 and np.array_equal(got, R.restatement(x, None, True, 128))
    grid = int(ctx.get_option("trace_fft_grid"))
    pack = max(1, min(512, 2048 // 8))  # the traces of a workgroup at N = 8 (include/alifmm.h)
    assert 1 <= grid <= 4096
    h = R.noise_response(8, 2)
    for ntrace in (2 * grid + 1, 2 * grid * pack + 1):
        x = R.noise((ntrace, 5), True, 32, f32=True)
        got = ctx.trace_spectral(x, response=h, analytic=True, nfft=8)
        assert np.array_equal(got, R.restatement(x, h, True, 8)), ntrace


# ---- 2. trace independence, repeatability ----

def test_trace_independence(ctx):
    x = R.noise((5, 1000), False, 41)
    h = R.noise_response(1024, 1)
    y = ctx.trace_spectral(x, response=h, analytic=True)
    assert np.array_equal(y, R.restatement(x, h, True))
    for k in range(5):  # a trace alone has the bits it has among the others
        assert np.array_equal(ctx.trace_spectral(x[k], response=h, analytic=True), y[k])
    assert np.array_equal(ctx.trace_spectral(x, response=h, analytic=True), y)  # and a second call's
    xn = x.copy()
    xn[2, 500] = np.nan  # a non-finite sample: that trace's output is unspecified, the others' bits stay
    yn = ctx.trace_spectral(xn, response=h, analytic=True)
    keep = [0, 1, 3, 4]
    assert np.array_equal(yn[keep], y[keep]) and np.isfinite(yn[keep]).all()


# ---- 3. errors ----

def _raw(ctx, ntrace, nt, ncomp, dtype, inp, nfft, resp_comp, resp, analytic, out):
    """alifmm_trace_spectral as declared, for the arguments the Python layer cannot express."""
    import _alifmm

    p = lambda a: None if a is None else a.ctypes.data
    rc = _alifmm.lib().alifmm_trace_spectral(ctx._h, ntrace, nt, ncomp, dtype, p(inp), nfft, resp_comp, p(resp), analytic,
                                             p(out))
    ctx._chk(rc, "trace_spectral")


def test_errors(ctx):
    """Every rejected input of the contract raises with rc=-2 and leaves out as it was; a valid call
    passes afterwards."""
    import _alifmm

    E = _alifmm.AlifmmError
    nt = 50
    x = R.noise((3, nt), False, 61)
    xc = np.ascontiguousarray(R.noise((3, nt), True, 62)).view(np.float64).reshape(3, nt, 2)
    big = np.zeros((1, 8193))
    h1 = R.noise_response(64, 1)
    h2 = np.ascontiguousarray(R.noise_response(64, 2)).view(np.float64).reshape(64, 2)
    hnan, hinf = h1.copy(), h2.copy()
    hnan[63] = np.nan
    hinf[5, 1] = np.inf
    out = np.full((3, nt, 2), 123.0)
    bad = [
        lambda: _raw(ctx, 3, nt, 1, 0, None, 64, 0, None, 1, out),   # null pointers
        lambda: _raw(ctx, 3, nt, 1, 0, x, 64, 0, None, 1, None),
        lambda: _raw(ctx, 3, nt, 2, 0, out, 64, 0, None, 1, out),    # out is in
        lambda: _raw(ctx, 0, nt, 1, 0, x, 64, 0, None, 1, out),      # ntrace
        lambda: _raw(ctx, -1, nt, 1, 0, x, 64, 0, None, 1, out),
        lambda: _raw(ctx, 3, 0, 1, 0, x, 64, 0, None, 1, out),       # nt
        lambda: _raw(ctx, 3, -1, 1, 0, x, 0, 0, None, 1, out),
        lambda: _raw(ctx, 1, 8193, 1, 0, big, 0, 0, None, 1, out),
        lambda: _raw(ctx, 3, nt, 0, 0, x, 64, 0, None, 1, out),      # ncomp
        lambda: _raw(ctx, 3, nt, 3, 0, x, 64, 0, None, 1, out),
        lambda: _raw(ctx, 3, nt, 1, -1, x, 64, 0, None, 1, out),     # dtype
        lambda: _raw(ctx, 3, nt, 1, 2, x, 64, 0, None, 1, out),
        lambda: _raw(ctx, 3, nt, 1, 0, x, 32, 0, None, 1, out),      # nfft: below nt, no power of two, beyond the cap
        lambda: _raw(ctx, 3, nt, 1, 0, x, 96, 0, None, 1, out),
        lambda: _raw(ctx, 3, nt, 1, 0, x, -64, 0, None, 1, out),
        lambda: _raw(ctx, 3, nt, 1, 0, x, 16384, 0, None, 1, out),
        lambda: _raw(ctx, 3, nt, 1, 0, x, 64, -1, h1, 1, out),       # resp_comp
        lambda: _raw(ctx, 3, nt, 1, 0, x, 64, 3, h1, 1, out),
        lambda: _raw(ctx, 3, nt, 1, 0, x, 64, 1, None, 1, out),      # resp NULL with resp_comp > 0, and the reverse
        lambda: _raw(ctx, 3, nt, 1, 0, x, 64, 2, None, 1, out),
        lambda: _raw(ctx, 3, nt, 1, 0, x, 64, 0, h1, 1, out),
        lambda: _raw(ctx, 3, nt, 1, 0, x, 64, 1, hnan, 1, out),      # a non-finite response value
        lambda: _raw(ctx, 3, nt, 2, 0, xc, 64, 2, hinf, 0, out),
        lambda: _raw(ctx, 3, nt, 1, 0, x, 64, 0, None, 2, out),      # analytic
        lambda: _raw(ctx, 3, nt, 1, 0, x, 64, 0, None, -1, out),
        lambda: _raw(ctx, 2 ** 62, nt, 1, 0, x, 64, 0, None, 1, out),  # more traces than 64-bit offsets hold
    ]
    for k, call in enumerate(bad):
        with pytest.raises(E, match="rc=-2"):
            call()
            pytest.fail("rejected input %d was accepted" % k)
    assert (out == 123.0).all()
    assert _alifmm.lib().alifmm_trace_spectral(None, 3, nt, 1, 0, x.ctypes.data, 64, 0, None, 1, out.ctypes.data) == -2
    assert (out == 123.0).all()
    # the Python layer's own checks
    with pytest.raises(ValueError, match="shape"):
        ctx.trace_spectral(np.float64(1.0))
    with pytest.raises(ValueError, match="response"):
        ctx.trace_spectral(x, response=np.ones(32))
    with pytest.raises(ValueError, match="response"):
        ctx.trace_spectral(x, response=np.ones((64, 1)))
    with pytest.raises(E, match="rc=-2"):
        ctx.trace_spectral(x, nfft=96)
    with pytest.raises(E, match="rc=-2"):
        ctx.trace_spectral(x[:0])
    # the context is still usable
    _raw(ctx, 3, nt, 1, 0, x, 64, 1, h1, 1, out)
    want = R.restatement(x, h1, True, 64)
    assert np.array_equal(out.view(np.complex128)[..., 0], want)
    assert np.array_equal(ctx.trace_spectral(x, response=h1, analytic=True), want)
