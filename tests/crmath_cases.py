"""The arguments on which csrc/cr_math.h is pinned, and their exact values.

Shared by tests/test_crmath.py (the host build) and tests/test_gpu_crmath.py (the device).  Every
argument is deterministic (seeded); every expected value comes from mpmath at PREC bits, rounded
once to float64 (round to nearest even, subnormals included).  The code under test never supplies an
expected value.

Two argument sets, each a dict of named groups in a fixed order:
  trig_groups()  for sin, cos, tan and sincos: all |x| < 2^14 (or non-finite), cr_math.h's own domain
  atan_groups()  for atan
and trig_big(): finite |x| >= 2^14, where cr_math.h hands over to libm (ocml on the device); the
bar there is an ulp bound (BIG_ULP), not bit equality.

hard(name): the committed arguments of tests/golden/crmath_hard.npz (tools/gen_crmath_hard.py),
whose exact value lies within 2^-63, relative, of a midpoint between adjacent doubles: closer than
the fast paths' tightest error bound, so a sound rounding test hands each to the double-double path.
"""
import functools
import math
import os

import numpy as np
from mpmath import libmp

HERE = os.path.dirname(os.path.abspath(__file__))
PREC = 200
FN = {"atan": 0, "sin": 1, "cos": 2, "tan": 3, "sincos": 4}  # alifmm_cr_math / oref_cr_batch numbering
HARD_FILE = os.path.join(HERE, "golden", "crmath_hard.npz")
HARD_KEYS = {"atan": ("atan_log", "atan_02"), "sin": ("sin_4pi", "sin_16k"), "cos": ("cos_4pi", "cos_16k"),
             "tan": ("tan_4pi", "tan_16k")}
HARD_BOUND = 2.0 ** -63
# OpenCL's documented accuracy of double sin / cos (4 ulp) and tan (5 ulp): the device's libm is ocml
BIG_ULP = {"sin": 4.0, "cos": 4.0, "tan": 5.0}
_RN = libmp.round_nearest


# ---- exact values ----
def _mpf(x):
    return libmp.from_float(float(x))


def _to_f64(v):
    """The mpf v rounded once to the nearest float64 (ties to even), subnormal results included."""
    sign, man, exp, bc = v
    if not man:
        return 0.0
    e = exp + bc  # 2^(e-1) <= |v| < 2^e
    prec = 53 if e - 53 >= -1074 else e + 1074
    if prec <= 0:  # below half the smallest subnormal, or a tie with zero
        half = (0, 1, -1075, 1)
        return math.copysign(5e-324 if libmp.mpf_cmp(libmp.mpf_abs(v), half) > 0 else 0.0, -1.0 if sign else 1.0)
    return libmp.to_float(libmp.mpf_pos(v, prec, _RN))


def _exact(fn, x):
    """The mpf values of fn at the finite double x: a tuple (atan,) or (sin, cos, tan)."""
    m = _mpf(x)
    if fn == "atan":
        return (libmp.mpf_atan(m, PREC),)
    c, s = libmp.mpf_cos_sin(m, PREC)
    return s, c, libmp.mpf_div(s, c, PREC)


def expected(fn, x):
    """fn in ("atan", "trig") at every element of x: atan -> one float64 array, trig -> (sin, cos,
    tan) arrays.  The sign of a zero result is the argument's; a non-finite argument gives NaN,
    except atan(+-inf) = +-fl(pi/2)."""
    x = np.asarray(x, dtype=np.float64)
    nout = 1 if fn == "atan" else 3
    out = [np.empty(x.shape) for _ in range(nout)]
    pio2 = _to_f64(libmp.mpf_shift(libmp.mpf_pi(PREC), -1))
    for i, xi in enumerate(x.tolist()):
        if xi != xi or xi in (math.inf, -math.inf):
            v = [math.copysign(pio2, xi) if fn == "atan" and xi == xi else math.nan] * nout
        elif xi == 0.0:
            v = [xi] if fn == "atan" else [xi, 1.0, xi]
        else:
            v = [_to_f64(m) for m in _exact(fn, xi)]
        for o, vi in zip(out, v):
            o[i] = vi
    return out[0] if fn == "atan" else tuple(out)


def midpoint_distance(fn, x):
    """|exact fn(x) - the nearest midpoint between adjacent doubles| / |exact fn(x)| for every finite,
    non-zero x with a normal result; fn in ("atan", "sin", "cos", "tan")."""
    which = {"atan": 0, "sin": 0, "cos": 1, "tan": 2}[fn]
    out = np.empty(len(x))
    for i, xi in enumerate(np.asarray(x, dtype=np.float64).tolist()):
        out[i] = _mid_dist(_exact("atan" if fn == "atan" else "trig", xi)[which])
    return out


def _mid_dist(v):
    sign, man, exp, bc = v
    sh = bc - 53  # bits below the float64 significand
    if sh < 2:  # the value is (nearly) a double itself: half an ulp from a midpoint
        return 2.0 ** -54
    low = man & ((1 << sh) - 1)
    d = abs(low - (1 << (sh - 1)))  # distance to the midpoint in units of 2^exp
    return libmp.to_float(libmp.mpf_div(libmp.from_man_exp(d, exp), libmp.mpf_abs(v), 64), rnd=_RN)


def ulp_error(got, want_mpf_fn, x):
    """max |got - exact| in ulps of the exact value's binade, over the finite doubles x;
    want_mpf_fn(xi) -> the exact mpf."""
    worst = 0.0
    for g, xi in zip(np.asarray(got).tolist(), np.asarray(x).tolist()):
        v = want_mpf_fn(xi)
        ulp_exp = v[2] + v[3] - 53
        err = libmp.mpf_abs(libmp.mpf_sub(_mpf(g), v, PREC)) if g == g and abs(g) != math.inf else libmp.finf
        worst = max(worst, float(libmp.to_float(libmp.mpf_shift(err, -ulp_exp))) if err != libmp.finf else math.inf)
    return worst


def big_ulp_error(fn, got, x):
    """Worst error in ulp of got = fn(x) (fn in sin / cos / tan) against mpmath."""
    which = {"sin": 0, "cos": 1, "tan": 2}[fn]
    return ulp_error(got, lambda xi: _exact("trig", xi)[which], x)


# ---- arguments ----
def _nb(v):
    """Every double of v with its two neighbouring doubles: [v, next below, next above] flattened."""
    v = np.asarray(v, dtype=np.float64).ravel()
    return np.stack([v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)], axis=1).ravel()


def _pm(v):
    return np.concatenate([v, -v])


@functools.lru_cache(maxsize=None)
def hard(name):
    """The committed hard arguments of one function: both of its scans, 2 x 1024 doubles."""
    with np.load(HARD_FILE) as z:
        return np.concatenate([z[k] for k in HARD_KEYS[name]])


def hard_scans():
    """(function, key, the 1024 arguments) of every scan of the fixture."""
    with np.load(HARD_FILE) as z:
        return [(f, k, z[k]) for f, keys in HARD_KEYS.items() for k in keys]


def _pi_mult(num, den):
    """fl(num pi / den) for the integer array num (mpmath, rounded once)."""
    pi = libmp.mpf_pi(PREC)
    return np.array([_to_f64(libmp.mpf_div(libmp.mpf_mul_int(pi, int(k), PREC), libmp.from_int(den), PREC)) for k in num])


@functools.lru_cache(maxsize=None)
def trig_groups():
    rng = np.random.default_rng(20240914)
    g = {}
    g["random_4pi"] = (rng.random(1 << 15) * 2 - 1) * (4 * np.pi)
    g["random_16k"] = (rng.random(1 << 15) * 2 - 1) * 16383.9
    # the grid of vmax_of and the velocity tables: deg pi/180, deg = 0, 0.05, ..., 360
    g["degrees"] = (np.arange(7201) * 0.05) * (np.pi / 180)
    # fl(k pi/2), all below 2^14: the worst cancellation of x - j pi/128, and tan at its poles
    g["pio2_multiples"] = _pm(_nb(_pi_mult(np.arange(1, 10431), 2)))
    # fl((j + 1/2) pi/128): the ties of nearbyint(x 128/pi)
    g["reduction_ties"] = _pm(_nb(_pi_mult(2 * np.arange(601) + 1, 256)))
    # x returned as is below 2^-26 (sin) / 2^-27 (tan); the hand-over to libm at 2^14 (from below:
    # 2^14 itself and beyond are trig_big()'s)
    g["thresholds"] = _pm(np.concatenate([_nb([2.0 ** -26, 2.0 ** -27]), [np.nextafter(2.0 ** 14, 0.0)]]))
    g["specials"] = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, np.inf, -np.inf, np.nan])
    for f in ("sin", "cos", "tan"):
        g["hard_" + f] = hard(f)
    return g


@functools.lru_cache(maxsize=None)
def atan_groups():
    rng = np.random.default_rng(20240915)
    g = {}
    g["random_log"] = np.exp2(rng.random(1 << 15) * 92 - 30) * rng.choice([-1.0, 1.0], 1 << 15)
    g["random_02"] = rng.random(1 << 15) * 2
    i, j = np.meshgrid(np.arange(1, 201, dtype=np.float64), np.arange(1, 201, dtype=np.float64), indexing="ij")
    g["int_ratios"] = (i / j).ravel()  # the source-init stencil angles atan(i / j)
    k = np.arange(129, dtype=np.float64)
    g["interval_bounds"] = _pm(_nb((k + 0.5) / 128))  # k = (int)(u 128 + 0.5) changes here
    g["interval_bounds_inv"] = _pm(_nb(128 / (k + 0.5)))  # the same through u = 1 / x
    g["thresholds"] = _pm(_nb([1.0, 256.0, 2.0 ** -27, 2.0 ** 60]))
    g["specials"] = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, np.inf, -np.inf, np.nan, 1e300, -1e300])
    g["hard_atan"] = hard("atan")
    return g


def trig_big():
    """Finite |x| >= 2^14: libm's domain (sin / cos / tan)."""
    rng = np.random.default_rng(20240916)
    v = np.concatenate([[2.0 ** 14, np.nextafter(2.0 ** 14, np.inf), 1e6, 1e22, 2.0 ** 60, 1e300],
                        np.exp2(14 + rng.random(500) * 1000)])
    return _pm(v)


def groups(kind):
    return atan_groups() if kind == "atan" else trig_groups()


@functools.lru_cache(maxsize=None)
def case_set(kind):
    """kind "atan" or "trig": (x, expected, slices).  x: all groups concatenated in their natural
    order; expected: expected(kind, x), computed once per process; slices: group name -> slice of x."""
    g = groups(kind)
    x = np.concatenate(list(g.values()))
    slices, o = {}, 0
    for name, v in g.items():
        slices[name] = slice(o, o + len(v))
        o += len(v)
    x.setflags(write=False)
    exp = expected(kind, x)
    for a in (exp,) if kind == "atan" else exp:
        a.setflags(write=False)
    return x, exp, slices


def hard_mask(fn):
    """The arguments of fn's case set that are hard for fn itself (sincos: for its sin or its cos)."""
    kind = "atan" if fn == "atan" else "trig"
    x, _, slices = case_set(kind)
    m = np.zeros(len(x), dtype=bool)
    for f in ("sin", "cos") if fn == "sincos" else (fn,):
        m[slices["hard_" + f]] = True
    return m


# ---- the host build of cr_math.h ----
def load_host():
    """oracle/lib/liboracle_cr.so (built when missing or stale) with oref_cr_batch declared."""
    import ctypes
    import subprocess

    repo = os.path.dirname(HERE)
    subprocess.check_call(["make", "-s", "-C", os.path.join(repo, "oracle"), "lib/liboracle_cr.so"])
    L = ctypes.CDLL(os.path.join(repo, "oracle", "lib", "liboracle_cr.so"))
    L.oref_cr_batch.restype = ctypes.c_int
    L.oref_cr_batch.argtypes = [ctypes.c_int, ctypes.c_longlong] + [ctypes.c_void_p] * 3
    return L


def host_batch(L, fn, x):
    """cr_math.h's fn ("atan", "sin", "cos", "tan": one array; "sincos": a pair) of every element of
    x, through the host build's batch entry point."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.full(x.shape, -77.0)
    out2 = np.full(x.shape, -77.0) if fn == "sincos" else None
    rc = L.oref_cr_batch(FN[fn], x.size, x.ctypes.data, out.ctypes.data, None if out2 is None else out2.ctypes.data)
    assert rc == 0, (fn, rc)
    return (out, out2) if fn == "sincos" else out


def same_bits(got, want):
    """Elementwise: got is want to the bit, the sign of zero included; any NaN equals any NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))


def describe_mismatches(x, got, want, limit=8):
    bad = np.nonzero(~same_bits(got, want))[0]
    return [(float(x[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:limit]]


def wave_order(is_hard, wave=64):
    """A permutation of the arguments for the device: first a block in which every run of `wave`
    consecutive arguments is all hard ones (a whole wave in the double-double path), then a block
    with a single hard argument per run among easy ones (one lane in it), then the rest in natural
    order.  Half of the hard arguments (whole runs) go to the first block."""
    hard_idx, easy_idx = np.nonzero(is_hard)[0], np.nonzero(~is_hard)[0]
    n_full = (len(hard_idx) // 2) // wave * wave
    lone = hard_idx[n_full:]
    n_lone = min(len(lone), len(easy_idx) // (wave - 1))
    lone, rest_hard = lone[:n_lone], lone[n_lone:]
    mixed = np.empty((n_lone, wave), dtype=np.int64)
    for r in range(n_lone):  # the hard one's lane moves through the wave
        mixed[r] = np.insert(easy_idx[r * (wave - 1):(r + 1) * (wave - 1)], r % wave, lone[r])
    rest = np.sort(np.concatenate([easy_idx[n_lone * (wave - 1):], rest_hard]))
    perm = np.concatenate([hard_idx[:n_full], mixed.ravel(), rest])
    assert len(perm) == len(is_hard) and len(np.unique(perm)) == len(perm)
    return perm
