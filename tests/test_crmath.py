"""The device's correctly rounded atan / sin / cos / tan (csrc/cr_math.h), on the host.

cr_math.h compiles for host and device; the oracle's CR build (oracle/lib/liboracle_cr.so)
exports it.  Checked here: (1) on random arguments every result is the correctly rounded value
(80-digit decimal reference, tools/gen_crmath_tables.py), (2) against glibc, the functions the
reference's numba code calls, results agree bitwise on all but a small fraction of arguments
(where glibc is off by just over half an ulp: printed by oracle/crcheck/crmath_check.cpp),
(3) on the case set of tests/crmath_cases.py (random, operator-domain, every reduction edge, the
committed hard arguments that only the double-double paths can round, specials) every result equals
the mpmath value rounded once, to the bit; beyond 2^14, libm's domain, an ulp bound holds instead.
tests/test_gpu_crmath.py runs the same set on the device.
"""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def cr():
    import crmath_cases as C

    L = C.load_host()
    for f in ("oref_cr_atan", "oref_cr_sin", "oref_cr_cos", "oref_cr_tan"):
        getattr(L, f).restype = ctypes.c_double
        getattr(L, f).argtypes = [ctypes.c_double]
    return L


def host_batch(L, fn, x):
    import crmath_cases as C

    return C.host_batch(L, fn, x)


@pytest.fixture(scope="module")
def D():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import gen_crmath_tables as G

    return G


def test_correctly_rounded(cr, D):
    from decimal import Decimal

    rng = np.random.default_rng(3)
    xs = np.concatenate([np.ldexp(1 + rng.random(150), rng.integers(-30, 30, 150)) * rng.choice([-1, 1], 150),
                         (rng.random(150) - 0.5) * 14])
    for x in xs:
        ref = float(D.atan(Decimal(float(x))))
        assert cr.oref_cr_atan(float(x)) == ref, ("atan", float(x).hex())
    P = D.PI
    for x in (rng.random(300) - 0.5) * 14:
        X = Decimal(float(x))
        k = (X / (2 * P)).to_integral_value()
        s = D.sin(X - 2 * P * k)
        c = D.sin(X - 2 * P * k + P / 2)
        assert cr.oref_cr_sin(float(x)) == float(s), ("sin", float(x).hex())
        assert cr.oref_cr_cos(float(x)) == float(c), ("cos", float(x).hex())
        if abs(c) > Decimal("1e-3"):
            assert cr.oref_cr_tan(float(x)) == float(s / c), ("tan", float(x).hex())


def test_agrees_with_glibc(tmp_path):
    exe = str(tmp_path / "crmath_check")
    subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=off", "-std=c++17", "-o", exe,
                           os.path.join(REPO, "oracle", "crcheck", "crmath_check.cpp"), "-lm"])
    r = json.loads(subprocess.check_output([exe, "300000"]))
    for name, v in r.items():
        assert v["mismatch"] <= 3e-3 * v["n"], (name, v)


def test_special_arguments(cr):
    inf = float("inf")
    assert cr.oref_cr_atan(inf) == math.atan(inf) and cr.oref_cr_atan(-inf) == math.atan(-inf)
    assert math.isnan(cr.oref_cr_atan(float("nan")))
    for f, g in ((cr.oref_cr_atan, math.atan), (cr.oref_cr_sin, math.sin), (cr.oref_cr_tan, math.tan)):
        for x in (0.0, -0.0, 1e-300, -3e-20, 5e-9):
            assert math.copysign(1, f(x)) == math.copysign(1, g(x)) and f(x) == g(x), (f, x)
    assert cr.oref_cr_cos(0.0) == 1.0 and cr.oref_cr_atan(1.0) == math.atan(1.0)
    assert cr.oref_cr_atan(1e300) == math.atan(1e300) and cr.oref_cr_sin(1e6) == math.sin(1e6)


# ---- the exact case set (tests/crmath_cases.py): every result against mpmath, to the bit ----
def test_case_set_reaches_the_edges():
    """The sets hold what they are meant to: the argument on which atan's interval choice went wrong,
    both table paths' edges, more arguments than a multiple of the device's workgroup."""
    import crmath_cases as C

    xa = C.case_set("atan")[0]
    xt = C.case_set("trig")[0]
    bad = float.fromhex("0x1.fffffffffffffp-9")
    assert bad in xa and -bad in xa
    for v in (1.0, 256.0, 2.0 ** -27, 2.0 ** 60, np.nextafter(2.0 ** 60, np.inf), 0.5 / 128, 128.5 / 128, 256.0 / 257):
        assert v in xa, v
    for v in (2.0 ** -26, 2.0 ** -27, np.nextafter(2.0 ** 14, 0), math.pi / 2, math.pi / 256, 10430 * (math.pi / 2)):
        assert v in xt or np.nextafter(v, 0) in xt or np.nextafter(v, np.inf) in xt, v
    assert np.all(~(np.abs(xt) >= 2.0 ** 14) | ~np.isfinite(xt))  # cr_math.h's own domain
    assert np.all(np.abs(C.trig_big()) >= 2.0 ** 14)
    assert len(xa) > 90000 and len(xt) > 90000 and len(xa) % 256 and len(xt) % 256


def test_hard_arguments_need_the_slow_path():
    """Every committed hard argument's exact value is within 2^-63 (relative) of a midpoint between
    adjacent doubles: closer than the fast paths' tightest error bound (atan's 2^-63 rounding test),
    so only the double-double paths can round it."""
    import crmath_cases as C

    assert os.path.getsize(C.HARD_FILE) <= 128 * 1024
    scans = C.hard_scans()
    assert len(scans) == 8
    for f, key, x in scans:
        assert x.dtype == np.float64 and x.shape == (1024,) and len(np.unique(x)) == 1024, key
        d = C.midpoint_distance(f, x)
        assert d.max() < C.HARD_BOUND, (key, float(x[d.argmax()]).hex(), d.max())


@pytest.mark.parametrize("fn", ["atan", "sin", "cos", "tan", "sincos"])
def test_exact_on_case_set(cr, fn):
    """Bit equality with the correctly rounded value on the whole case set: random and operator-domain
    arguments, every reduction edge, the hard arguments and the specials (signs of zero, NaN-ness)."""
    import crmath_cases as C

    kind = "atan" if fn == "atan" else "trig"
    x, exp, slices = C.case_set(kind)
    got = host_batch(cr, fn, x)
    pairs = {"atan": [(got, exp)], "sincos": [(got[0], exp[0]), (got[1], exp[1])]}.get(fn) or \
        [(got, exp[("sin", "cos", "tan").index(fn)])]
    for g, e in pairs:
        ok = C.same_bits(g, e)
        bad_groups = [n for n, s in slices.items() if not ok[s].all()]
        assert ok.all(), (fn, int((~ok).sum()), bad_groups, C.describe_mismatches(x, g, e))
    if fn == "sincos":  # one reduction, the same results as the separate calls
        assert C.same_bits(got[0], host_batch(cr, "sin", x)).all()
        assert C.same_bits(got[1], host_batch(cr, "cos", x)).all()
    # the batch entry point is the per-argument one
    f1 = {"atan": cr.oref_cr_atan, "sin": cr.oref_cr_sin, "cos": cr.oref_cr_cos, "tan": cr.oref_cr_tan}.get(fn)
    if f1:
        sub = np.arange(0, len(x), 97)
        assert C.same_bits(got[sub], np.array([f1(float(v)) for v in x[sub]])).all()


@pytest.mark.parametrize("fn", ["sin", "cos", "tan"])
def test_beyond_2p14_follows_libm(cr, fn):
    """|x| >= 2^14 is libm's (glibc here, ocml on the device): held to OpenCL's documented bound for
    double sin / cos (4 ulp) and tan (5 ulp) against mpmath, on both."""
    import crmath_cases as C

    x = C.trig_big()
    worst = C.big_ulp_error(fn, host_batch(cr, fn, x), x)
    print("host %s beyond 2^14: worst %.3f ulp over %d arguments" % (fn, worst, len(x)))
    assert worst <= C.BIG_ULP[fn], (fn, worst)


def test_batch_rejects_bad_calls(cr):
    x = np.array([0.5])
    out = np.full(1, -77.0)
    assert cr.oref_cr_batch(5, 1, x.ctypes.data, out.ctypes.data, out.ctypes.data) == -1
    assert cr.oref_cr_batch(-1, 1, x.ctypes.data, out.ctypes.data, out.ctypes.data) == -1
    assert cr.oref_cr_batch(4, 1, x.ctypes.data, out.ctypes.data, None) == -1
    assert out[0] == -77.0


def test_case_set_under_sanitizers(tmp_path):
    """The whole case set through a stand-alone program (oracle/crcheck/cr_batch_main.cpp + the
    batch shim) built with AddressSanitizer and UBSan: a clean run (out-of-range table indices,
    (int) of an unrepresentable value and the like would abort it) with the exact results."""
    import crmath_cases as C

    exe = str(tmp_path / "cr_batch_san")
    d = os.path.join(REPO, "oracle", "crcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-mfma", "-ffp-contract=off", "-std=c++17",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(d, "cr_batch_main.cpp"), os.path.join(d, "cr_shim.cpp")])
    # (no leak check at exit: it needs ptrace, which a sandboxed test machine may not allow)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    for fn in ("atan", "sincos", "tan"):
        x, exp, _ = C.case_set("atan" if fn == "atan" else "trig")
        x = np.concatenate([x, C.trig_big()]) if fn != "atan" else x
        fin, fout = str(tmp_path / (fn + ".in")), str(tmp_path / (fn + ".out"))
        x.tofile(fin)
        r = subprocess.run([exe, str(C.FN[fn]), fin, fout], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (fn, r.returncode, r.stderr[-2000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (fn, r.stderr[-2000:])
        got = np.fromfile(fout).reshape(-1, len(x))[:, :len(exp if fn == "atan" else exp[0])]
        want = [exp] if fn == "atan" else [exp[0], exp[1]] if fn == "sincos" else [exp[2]]
        for g, e in zip(got, want):
            assert C.same_bits(g, e).all(), (fn, C.describe_mismatches(x, g, e))
