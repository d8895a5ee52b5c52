"""GPU tests of the trace FIR and its transpose (include/alifmm.h alifmm_trace_fir; csrc/trace_fir.hip,
the sum of csrc/trace_fir_term.h) against the numpy restatement tests/trace_fir_ref.py.  The contract
fixes the order of every operation, so the comparisons are equalities of bits (np.array_equal), not
tolerances; only the adjoint identity, which compares two different sums, has a bar
(trace_fir_ref.adjoint_bar, derived there).  The measured figures go to the session's envelope under
trace_fir/... ."""
import numpy as np
import pytest

import trace_fir_ref as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)  # no model: the FIR needs none
    yield c
    c.close()


# ---- 1. bit equality against the restatement ----

@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("name,cplx_data,cplx_taps", F.TYPES)
def test_bits_against_the_restatement(ctx, name, cplx_data, cplx_taps, transpose):
    """Seeded float64 noise, 3 traces: traces of 1 and 2 samples, a tile less one, a tile, a tile
    and one, two tiles and three; 1, 2, 17 and 1024 taps (a halo as long as a tile, a pulse longer
    than the trace, the cap), and tile + 5 where the cap allows it; the origin at the first, the
    middle and the last tap."""
    T = int(ctx.get_option("trace_fir_tile"))
    assert T >= 4 and T % 4 == 0
    shapes = F.shapes(T)
    assert {s[1] for s in shapes} >= {1, 2, 17, 1024} and {s[0] for s in shapes} == {1, 2, T - 1, T, T + 1, 2 * T + 3}
    for nt, ntap, origin in shapes:
        x = F.noise((3, nt), cplx_data, 100 + nt)
        h = F.noise_taps(ntap, cplx_taps)
        got = ctx.trace_fir(x, h, origin=origin, transpose=transpose)
        want = F.fir_ref(x, h, origin, transpose)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert np.array_equal(got, want), (nt, ntap, origin, np.abs(got - want).max())
        assert want.any()
    assert ctx.get_option("trace_fir_kernel_ms") > 0 and ctx.get_option("trace_fir_upload_ms") > 0


@pytest.mark.parametrize("transpose", [False, True])
def test_bits_on_many_traces(ctx, transpose):
    """65 x 65 traces of 480 complex samples, 17 complex taps: more (trace, tile) pairs than the
    launch has workgroups, so every workgroup walks its share with the grid's stride."""
    x = F.noise((65, 65, 480), True, 31)
    h = F.pulse(17, 3, True)
    got = ctx.trace_fir(x, h, origin=8, transpose=transpose)
    assert got.shape == x.shape and np.array_equal(got, F.fir_ref(x, h, 8, transpose))


# ---- 2. trace independence, repeatability, in place ----

def _raw(ctx, ntrace, nt, ncomp, inp, ntap, tap_comp, taps, origin, transpose, out):
    """alifmm_trace_fir as declared, for the arguments the Python layer cannot express."""
    import _alifmm

    p = lambda a: None if a is None else a.ctypes.data
    rc = _alifmm.lib().alifmm_trace_fir(ctx._h, ntrace, nt, ncomp, p(inp), ntap, tap_comp, p(taps), origin, transpose,
                                        p(out))
    ctx._chk(rc, "trace_fir")


def test_trace_independence_and_in_place(ctx):
    T = int(ctx.get_option("trace_fir_tile"))
    nt = T + 37
    x = F.noise((5, nt), True, 41)
    h = F.pulse(33, 5, True)
    for transpose in (False, True):
        y = ctx.trace_fir(x, h, origin=16, transpose=transpose)
        for k in range(5):  # a trace alone has the bits it has among the others
            assert np.array_equal(ctx.trace_fir(x[k], h, origin=16, transpose=transpose), y[k])
        assert np.array_equal(ctx.trace_fir(x, h, origin=16, transpose=transpose), y)  # and a second call's
        buf = np.ascontiguousarray(x).view(np.float64).reshape(5, nt, 2).copy()
        taps = np.ascontiguousarray(h).view(np.float64).reshape(-1, 2)
        _raw(ctx, 5, nt, 2, buf, 33, 2, taps, 16, int(transpose), buf)  # out is in
        assert np.array_equal(buf.view(np.complex128)[..., 0], y)
    # a non-finite sample propagates to the outputs it reaches and no further
    xn = x.real.copy()
    xn[2, 500] = np.nan
    yn = ctx.trace_fir(xn, h.real, origin=16)
    assert np.array_equal(yn, F.fir_ref(xn, h.real, 16), equal_nan=True)
    assert np.isnan(yn[2]).sum() == 33 and np.isfinite(np.delete(yn, 2, axis=0)).all()


# ---- 3. adjointness ----

@pytest.mark.parametrize("name,cplx_data,cplx_taps", F.TYPES)
def test_adjoint_identity(ctx, envelope, name, cplx_data, cplx_taps):
    """|<P x, y> - <x, Pᵀ y>| under trace_fir_ref.adjoint_bar, and far above it with one tap changed."""
    T = int(ctx.get_option("trace_fir_tile"))
    nt, ntap, origin = 2 * T + 3, 64, 20
    x, y = F.noise((4, nt), cplx_data, 51), F.noise((4, nt), cplx_data, 52)
    h = F.pulse(ntap, 6, cplx_taps)
    lhs = F.real_dot(ctx.trace_fir(x, h, origin=origin), y)
    rhs = F.real_dot(x, ctx.trace_fir(y, h, origin=origin, transpose=True))
    bar, S = F.adjoint_bar(x, y, h, origin)
    envelope["trace_fir/adjoint_" + name] = abs(lhs - rhs) / bar
    print("trace_fir/adjoint_%s: |<Px, y> - <x, P^T y>| / bar = %.3g (lhs %.6g, S %.3g)" % (name, abs(lhs - rhs) / bar, lhs, S))
    assert abs(lhs - rhs) <= bar
    h2 = h.copy()
    h2[40] = 0
    assert abs(F.real_dot(ctx.trace_fir(x, h2, origin=origin), y) - rhs) > 1e3 * bar


# ---- 4. errors ----

def test_errors(ctx):
    """Every rejected input of the contract raises with rc=-2 and leaves out as it was; a valid call
    passes afterwards."""
    import _alifmm

    E = _alifmm.AlifmmError
    nt = 50
    x = F.noise((3, nt), True, 61)
    h = F.pulse(17, 3, True)
    bad = [
        lambda: ctx.trace_fir(x, np.zeros(0)),                      # ntap < 1
        lambda: ctx.trace_fir(x, np.ones(1025)),                    # ntap > ALIFMM_FIR_MAX_TAPS
        lambda: ctx.trace_fir(x, 1j * np.ones(1025)),
        lambda: ctx.trace_fir(x, h, origin=-1),                     # origin
        lambda: ctx.trace_fir(x, h, origin=17),
        lambda: ctx.trace_fir(x, np.array([1.0, np.nan, 1.0])),     # a non-finite tap
        lambda: ctx.trace_fir(x, np.array([1.0, 1.0, complex(0, np.inf)])),
        lambda: ctx.trace_fir(x[:0], h),                            # ntrace < 1
        lambda: ctx.trace_fir(x[:, :0], h),                         # nt < 1
    ]
    xs = np.ascontiguousarray(x).view(np.float64).reshape(3, nt, 2)
    taps = np.ascontiguousarray(h).view(np.float64).reshape(-1, 2)
    out = np.full(xs.shape, 123.0)
    bad += [
        lambda: _raw(ctx, 3, nt, 2, None, 17, 2, taps, 0, 0, out),  # null pointers
        lambda: _raw(ctx, 3, nt, 2, xs, 17, 2, None, 0, 0, out),
        lambda: _raw(ctx, 3, nt, 2, xs, 17, 2, taps, 0, 0, None),
        lambda: _raw(ctx, 0, nt, 2, xs, 17, 2, taps, 0, 0, out),    # ntrace, nt
        lambda: _raw(ctx, -1, nt, 2, xs, 17, 2, taps, 0, 0, out),
        lambda: _raw(ctx, 3, 0, 2, xs, 17, 2, taps, 0, 0, out),
        lambda: _raw(ctx, 3, nt, 0, xs, 17, 1, taps, 0, 0, out),    # ncomp, tap_comp
        lambda: _raw(ctx, 3, nt, 3, xs, 17, 1, taps, 0, 0, out),
        lambda: _raw(ctx, 3, nt, 2, xs, 17, 0, taps, 0, 0, out),
        lambda: _raw(ctx, 3, nt, 2, xs, 17, 3, taps, 0, 0, out),
        lambda: _raw(ctx, 3, nt, 1, xs, 17, 2, taps, 0, 0, out),    # complex taps on real data
        lambda: _raw(ctx, 3, nt, 2, xs, 0, 2, taps, 0, 0, out),     # ntap
        lambda: _raw(ctx, 3, nt, 2, xs, 1025, 2, taps, 0, 0, out),
        lambda: _raw(ctx, 3, nt, 2, xs, 17, 2, taps, 17, 0, out),   # origin
        lambda: _raw(ctx, 3, nt, 2, xs, 17, 2, taps, -1, 0, out),
        lambda: _raw(ctx, 3, nt, 2, xs, 17, 2, taps, 0, 2, out),    # transpose
        lambda: _raw(ctx, 3, nt, 2, xs, 17, 2, taps, 0, -1, out),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(E, match="rc=-2"):
            call()
            pytest.fail("rejected input %d was accepted" % k)
    assert (out == 123.0).all()
    assert _alifmm.lib().alifmm_trace_fir(None, 3, nt, 2, xs.ctypes.data, 17, 2, taps.ctypes.data, 0, 0, out.ctypes.data) == -2
    assert (out == 123.0).all()
    # the Python layer's own checks
    with pytest.raises(ValueError, match="complex pulse"):
        ctx.trace_fir(x.real, h)
    with pytest.raises(ValueError):
        ctx.trace_fir(x, np.ones((2, 2)))
    with pytest.raises(ValueError):
        ctx.trace_fir(np.float64(1.0), h.real)
    # the context is still usable
    _raw(ctx, 3, nt, 2, xs, 17, 2, taps, 8, 0, out)
    assert np.array_equal(out.view(np.complex128)[..., 0], F.fir_ref(x, h, 8))
    assert np.array_equal(ctx.trace_fir(x, h, origin=8), F.fir_ref(x, h, 8))
