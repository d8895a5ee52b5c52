"""csrc/cr_math.h on the device, against exact values.

alifmm_cr_math evaluates atan / sin / cos / tan / sincos one argument per thread through the macros
the operators use, with the tables read from global constants (lds_tables 0, utils.hip) or from LDS
after crm::lds_init() (lds_tables 1, cr_eval.hip: the solver and ray kernels' configuration).  Each
function runs the whole case set of tests/crmath_cases.py in one launch and must equal, to the bit,
the mpmath value rounded once and the host build's result (tests/test_crmath.py pins the latter to
the former).  The arguments are ordered so that both divergence patterns of the double-double paths
occur: whole waves of hard arguments, then one hard lane per wave, then the rest.  Beyond 2^14 the
functions are libm's (ocml here): held to OpenCL's documented ulp bound, worst ulp recorded.
"""
import numpy as np
import pytest

import crmath_cases as C

pytestmark = pytest.mark.gpu

FNS = ("atan", "sin", "cos", "tan", "sincos")


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host():
    return C.load_host()


def _want(fn, exp):
    return {"atan": [exp], "sincos": [exp[0], exp[1]]}.get(fn) or [exp[("sin", "cos", "tan").index(fn)]]


@pytest.mark.parametrize("lds", [0, 1])
@pytest.mark.parametrize("fn", FNS)
def test_device_exact_on_case_set(ctx, host, envelope, fn, lds):
    x, exp, slices = C.case_set("atan" if fn == "atan" else "trig")
    hard = C.hard_mask(fn)
    perm = C.wave_order(hard)
    n_full = (int(hard.sum()) // 2) // 64 * 64
    assert n_full >= 512 and hard[perm[:n_full]].all()  # whole waves in the slow path
    assert (hard[perm[n_full:n_full + 64 * 256]].reshape(-1, 64).sum(axis=1) == 1).all()  # one lane of a wave
    assert len(x) % 256 != 0 and len(x) > 256 * 256
    xs = x[perm]
    got = ctx.cr_math(fn, xs, lds_tables=bool(lds))
    got = list(got) if fn == "sincos" else [got]
    hst = C.host_batch(host, fn, xs)
    hst = list(hst) if fn == "sincos" else [hst]
    mism = mism_host = 0
    report = []
    for g, h, e in zip(got, hst, _want(fn, exp)):
        gn = np.empty_like(g)
        gn[perm] = g
        ok = C.same_bits(gn, e)
        mism += int((~ok).sum())
        mism_host += int((~C.same_bits(g, h)).sum())
        if not ok.all():
            report.append(([n for n, s in slices.items() if not ok[s].all()], C.describe_mismatches(x, gn, e)))
    envelope["crmath/%s_lds%d" % (fn, lds)] = {"n": int(len(x)), "mismatch": mism, "mismatch_host": mism_host}
    print("crmath %s lds %d: %d arguments, %d differ from exact, %d from the host" % (fn, lds, len(x), mism, mism_host))
    assert mism == 0, (fn, lds, mism, report)
    assert mism_host == 0, (fn, lds, mism_host)


@pytest.mark.parametrize("lds", [0, 1])
def test_sincos_is_sin_and_cos(ctx, lds):
    """fn 4 returns exactly what fn 1 and fn 2 return."""
    x = C.case_set("trig")[0]
    s, c = ctx.cr_math("sincos", x, bool(lds))
    assert C.same_bits(s, ctx.cr_math("sin", x, bool(lds))).all()
    assert C.same_bits(c, ctx.cr_math("cos", x, bool(lds))).all()


@pytest.mark.parametrize("lds", [0, 1])
def test_device_beyond_2p14_within_ocml_bound(ctx, envelope, lds):
    x = C.trig_big()
    s2, c2 = ctx.cr_math("sincos", x, bool(lds))
    rec = {}
    for fn in ("sin", "cos", "tan"):
        got = ctx.cr_math(fn, x, bool(lds))
        rec[fn] = C.big_ulp_error(fn, got, x)
        if fn != "tan":
            assert C.same_bits(got, s2 if fn == "sin" else c2).all()
    envelope["crmath/beyond_2p14_ulp_lds%d" % lds] = dict(rec, n=int(len(x)))
    print("crmath beyond 2^14, lds %d: worst ulp %s over %d arguments" % (lds, rec, len(x)))
    for fn, w in rec.items():
        assert w <= C.BIG_ULP[fn], (fn, lds, w)


def test_shapes_and_empty(ctx):
    assert ctx.cr_math("atan", np.empty(0)).shape == (0,)
    s, c = ctx.cr_math("sincos", np.empty(0), lds_tables=True)
    assert s.shape == (0,) and c.shape == (0,)
    x = np.linspace(-3, 3, 2 * 3 * 5).reshape(2, 3, 5)
    for lds in (False, True):
        a = ctx.cr_math(0, x, lds)
        assert a.shape == x.shape and C.same_bits(a, C.expected("atan", x.ravel()).reshape(x.shape)).all()
    # exactly one workgroup, one more, one less: the last block's bound
    xe, ee = C.case_set("atan")[:2]
    for n in (255, 256, 257):
        for lds in (False, True):
            assert C.same_bits(ctx.cr_math("atan", xe[:n], lds), ee[:n]).all(), (n, lds)


def test_error_cases(ctx):
    """Every refusal is ALIFMM_E_ARG with a message naming cr_math and leaves the outputs alone;
    a valid call on the same context follows each."""
    import _alifmm

    L = _alifmm.lib()
    E_ARG = -2  # ALIFMM_E_ARG (include/alifmm.h)
    x = np.array([0.25, -3.0, 100.0])
    want = C.expected("atan", x)
    ws, wc, _ = C.expected("trig", x)
    null = None

    def raw(fn, lds, n, xp, op, o2p):
        return L.alifmm_cr_math(ctx._h, fn, lds, n, xp, op, o2p)

    def valid():
        assert C.same_bits(ctx.cr_math("atan", x), want).all()
        s, c = ctx.cr_math("sincos", x, lds_tables=True)
        assert C.same_bits(s, ws).all() and C.same_bits(c, wc).all()

    out, out2 = np.full(3, -77.0), np.full(3, -77.0)
    px, po, po2 = x.ctypes.data, out.ctypes.data, out2.ctypes.data
    bad = [(5, 0, 3, px, po, po2), (-1, 0, 3, px, po, po2), (0, 2, 3, px, po, po2), (0, -1, 3, px, po, po2),
           (0, 0, -1, px, po, po2), (0, 1, 3, null, po, po2), (1, 0, 3, px, null, po2), (4, 1, 3, px, po, null),
           (4, 0, 3, px, null, po2)]
    for args in bad:
        assert raw(*args) == E_ARG, args
        msg = L.alifmm_last_error(ctx._h).decode()
        assert "cr_math" in msg, (args, msg)
        assert (out == -77.0).all() and (out2 == -77.0).all(), args
        valid()
    # out2 is ignored for fn 0 .. 3; n = 0 succeeds with nothing written, null pointers included
    assert raw(0, 0, 3, px, po, null) == 0 and C.same_bits(out, want).all()
    out[:] = -77.0
    assert raw(4, 1, 0, null, null, null) == 0 and raw(0, 0, 0, px, po, po2) == 0
    assert (out == -77.0).all() and (out2 == -77.0).all()
    with pytest.raises(_alifmm.AlifmmError, match="cr_math"):
        ctx.cr_math(7, x)
    with pytest.raises(_alifmm.AlifmmError, match="cr_math.*foo"):
        ctx.cr_math("foo", x)
    with pytest.raises(_alifmm.AlifmmError, match="cr_math"):
        ctx.cr_math("sin", x, lds_tables=2)
    valid()
