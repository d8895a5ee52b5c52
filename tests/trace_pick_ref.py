"""numpy restatement of the time-of-flight picker's contract of include/alifmm.h (alifmm_trace_pick),
the case set of the bit-equality tests and the files of the stand-alone host program
tests/trace_pick_sim.cpp.  Test infrastructure only.

pick_trace() is the contract rule by rule on one trace, scalar and plain: the energies are formed
with one numpy operation per product and per sum (nothing contracts), every comparison, square root
(math.sqrt, correctly rounded) and division then runs on Python floats, and both searches are loops
over the gate in ascending order.  There is no reduction tree here, and none is needed: the order
the picks are the maximum of is total.  So the device's outputs equal these bit for bit.
"""
import math

import numpy as np

NO_GATE, EMPTY, UNREFINED, AT_EDGE, NON_FINITE = 1, 2, 4, 8, 16
NAMES = ("pos", "amp", "idx", "amp2", "idx2", "flags")


def energy(x):
    """e[n] = (re * re) + (im * im), x * x for real data, in float64."""
    x = np.asarray(x)
    with np.errstate(all="ignore"):
        if np.iscomplexobj(x):
            re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
            rr, ii = re * re, im * im
            return rr + ii
        re = x.astype(np.float64)
        return re * re


def finite(e):
    """Neither NaN nor +-inf, on the bits: the exponent field is not all ones."""
    b = np.ascontiguousarray(e, dtype=np.float64).view(np.uint64)
    return (b & np.uint64(0x7ff0000000000000)) != np.uint64(0x7ff0000000000000)


def _none(flags):
    return (math.nan, 0.0, -1, 0.0, -1, flags)


def pick_trace(x, lo, hi, mode=0, frac=0.5, guard=0):
    """(pos, amp, idx, amp2, idx2, flags) of one trace x (nt,) and the gate [lo, hi)."""
    nt = len(x)
    assert mode in (0, 1) and guard >= 0 and (mode == 0 or 0 < frac <= 1)
    if lo >= hi:
        return _none(NO_GATE)
    assert 0 <= lo and hi <= nt
    ea = energy(x)
    e, ok = ea.tolist(), finite(ea).tolist()
    flags = 0
    idx = -1
    for n in range(lo, hi):
        if not ok[n]:
            flags |= NON_FINITE
        elif idx < 0 or e[n] > e[idx]:  # ascending n: of equal energies the lower index stays
            idx = n
    if idx < 0 or e[idx] == 0.0:
        return _none(flags | EMPTY)
    amp = math.sqrt(e[idx])
    idx2 = -1
    for n in range(lo, hi):
        if ok[n] and abs(n - idx) > guard and (idx2 < 0 or e[n] > e[idx2]):
            idx2 = n
    amp2 = math.sqrt(e[idx2]) if idx2 >= 0 else 0.0
    delta, refined = 0.0, False
    if mode == 0:
        m = idx
        if 0 < m < nt - 1 and ok[m - 1] and ok[m + 1]:
            am, a0, ap = math.sqrt(e[m - 1]), amp, math.sqrt(e[m + 1])
            if am <= a0 and ap <= a0:
                den = (am - (2.0 * a0)) + ap
                if den < 0.0:
                    delta = (0.5 * (am - ap)) / den
                    refined = True
        if m == lo or m == hi - 1:
            flags |= AT_EDGE
    else:
        thr = (frac * frac) * e[idx]
        m = next(n for n in range(lo, hi) if ok[n] and e[n] >= thr)
        if m > 0 and ok[m - 1] and e[m - 1] < thr:
            at, a1, am = math.sqrt(thr), math.sqrt(e[m]), math.sqrt(e[m - 1])
            den = a1 - am
            if den > 0.0:
                delta = -((a1 - at) / den)
                refined = True
        if m == lo:
            flags |= AT_EDGE
    if not refined:
        flags |= UNREFINED
    return (float(m) + delta, amp, idx, amp2, idx2, flags)


def pick(data, gate_lo, gate_hi, mode=0, frac=0.5, guard=0):
    """pick_trace() over data (..., nt) with gates shaped like the leading dimensions: (pos, amp,
    idx, amp2, idx2, flags), float64 and int32 arrays of that shape."""
    data = np.asarray(data)
    lead = data.shape[:-1]
    x = data.reshape(-1, data.shape[-1])
    lo, hi = np.broadcast_to(gate_lo, lead).ravel(), np.broadcast_to(gate_hi, lead).ravel()
    rows = [pick_trace(x[t], int(lo[t]), int(hi[t]), mode, frac, guard) for t in range(x.shape[0])]
    return tuple(np.array([r[k] for r in rows], dtype=np.float64 if k in (0, 1, 3) else np.int32).reshape(lead)
                 for k in range(6))


def same_bits(got, want):
    """Every one of the six outputs equal to the bit (NaN positions included)."""
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype != w.dtype or g.shape != w.shape:
            return False, "%s: %s %s against %s %s" % (name, g.dtype, g.shape, w.dtype, w.shape)
        kind = np.uint64 if g.dtype == np.float64 else np.int32
        bad = np.nonzero(np.ascontiguousarray(g).view(kind).ravel() != np.ascontiguousarray(w).view(kind).ravel())[0]
        if len(bad):
            k = int(bad[0])
            return False, "%s[%d]: %r against %r (%d differ)" % (name, k, g.ravel()[k], w.ravel()[k], len(bad))
    return True, ""


# ---- the case set ----

def _noise(rng, nt, cplx):
    d = 0.25 * rng.standard_normal(nt)
    return d + 0.25j * rng.standard_normal(nt) if cplx else d


def _pulse(nt, centre, cplx):
    """A Gaussian-modulated pulse (sigma 6 samples, 0.1 cycles per sample) around `centre`."""
    k = np.arange(nt) - centre
    env = 3.0 * np.exp(-0.5 * (k / 6.0) ** 2)
    return env * np.exp(2j * np.pi * 0.1 * k) if cplx else env * np.cos(2 * np.pi * 0.1 * k)


def _designs(nt):
    """The designed traces of a length: (edit(x, v), lo, hi); v is a value whose energy exceeds the
    noise's and 2 v one that exceeds that."""
    def put(**at):
        def edit(x, v):
            for k, val in at.items():
                x[int(k[1:])] = val if isinstance(val, float) and not np.isfinite(val) else val * v
        return edit

    def span(a, b, val):
        def edit(x, v):
            x[a:b] = val if not np.isfinite(val) else val * v
        return edit

    keep = lambda x, v: None
    if nt == 1:
        return [(put(n0=1.0), 0, 1), (span(0, 1, 0.0), 0, 1), (keep, 0, 0), (put(n0=np.nan), 0, 1), (keep, 1, 0)]
    if nt == 2:
        return [(keep, 0, 2), (keep, 0, 1), (keep, 1, 2), (put(n1=1.0), 0, 2), (put(n0=1.0, n1=1.0), 0, 2),
                (put(n0=np.inf), 0, 2), (keep, 2, 2)]
    if nt == 65:
        return [(keep, 0, 65), (keep, 0, 64), (keep, 1, 65), (keep, 64, 65), (put(n0=1.0, n64=1.0), 0, 65),
                (put(n64=1.0), 0, 65), (put(n0=1.0), 0, 65), (put(n63=1.0), 0, 64)]
    assert nt == 300
    return [
        (keep, 10, 11),                                  # a gate of 1 sample
        (keep, 5, 68), (keep, 5, 69), (keep, 5, 70),     # 63, 64, 65 samples
        (keep, 100, 229),                                # 129 samples
        (keep, 0, 300),                                  # the whole trace
        (put(n0=1.0), 0, 40),                            # the peak on sample 0
        (put(n299=1.0), 250, 300),                       # ... and on sample nt - 1
        (put(n30=1.0, n95=1.0), 20, 200),                # equal maxima 65 apart: different lanes
        (put(n159=1.0, n30=1.0), 20, 200),               # ... and 129 apart
        (put(n31=1.0, n160=1.0, n225=1.0), 20, 230),     # three of them
        (span(50, 60, 1.0), 20, 120),                    # a plateau
        (span(100, 150, 0.0), 100, 150),                 # an all-zero gate
        (put(n120=np.nan, n130=np.inf, n140=-np.inf), 100, 229),  # non-finite samples are not picked
        (span(100, 229, np.nan), 100, 229),              # a gate that is all NaN
        (span(100, 229, np.nan), 90, 229),               # ... but for ten samples
        (keep, 50, 50), (keep, 60, 40), (keep, 300, 300), (keep, 0, 0),  # no gate
        (put(n149=1.0, n150=2.0), 100, 150),             # the peak at hi - 1, a larger sample beyond
        (put(n100=1.0, n99=2.0), 100, 150),              # the peak at lo, a larger sample before
        (put(n100=1.0, n99=np.nan), 100, 150),           # ... a NaN before
        (put(n110=1.0), 107, 115),                       # 8 samples: guard 7 covers the gate
        (put(n110=1.0, n111=1.0), 100, 150),             # a flat top of two: den < 0, delta = -0.5
        (put(n110=1e200), 100, 150),                     # an energy that overflows (float32: an inf sample)
        ("pulse", 100, 229), ("pulse", 148, 229), ("pulse", 156, 229), ("pulse", 100, 151),  # onset at lo, cut echoes
    ]


def case_set(nt, ntrace, cplx, f32, seed=0):
    """(data (ntrace, nt), lo, hi): trace k is design k mod the number of designs of this length on
    noise of its own (a seeded quarter-unit normal), so every count reaches every design it can."""
    designs = _designs(nt)
    data = np.empty((ntrace, nt), dtype=np.complex128 if cplx else np.float64)
    lo, hi = np.empty(ntrace, dtype=np.int32), np.empty(ntrace, dtype=np.int32)
    for k in range(ntrace):
        rng = np.random.default_rng(1000 * seed + 7 * nt + k)
        edit, lo[k], hi[k] = designs[k % len(designs)]
        x = _noise(rng, nt, cplx)
        if isinstance(edit, str):
            x = x * 0.01 + _pulse(nt, 160.3 + 0.1 * (k // len(designs)), cplx)
        else:
            edit(x, (3.0 - 4.0j) if cplx else -5.0)
        data[k] = x
    with np.errstate(all="ignore"):
        if f32:
            data = data.astype(np.complex64 if cplx else np.float32)
    return data, lo, hi


SHAPES = ((1, 1), (2, 3), (65, 5), (300, 67))  # (nt, ntrace)
TYPES = tuple((cplx, f32) for cplx in (False, True) for f32 in (False, True))
MODES = ((0, 0.5), (1, 0.5), (1, 1.0))  # (mode, frac)
GUARDS = (0, 7)


def whole_trace_case(cplx, f32, nt=8192):
    """One trace of nt samples of seeded noise and its whole-trace gate."""
    x = _noise(np.random.default_rng(77), nt, cplx)[None]
    x = x.astype((np.complex64 if cplx else np.float32) if f32 else x.dtype)
    return x, np.zeros(1, dtype=np.int32), np.full(1, nt, dtype=np.int32)


# ---- gates from predicted times (ALI_FMM.pick_times) is tested against this plain loop ----

def gates_ref(around, half_width, t0, fs, nt):
    """Per entry of around: the samples n with |t0 + n / fs - around| <= half_width, clipped to
    0 .. nt - 1, as [lo, hi); NaN or nothing inside: lo = hi = 0."""
    around = np.asarray(around, dtype=np.float64)
    lo, hi = np.zeros(around.shape, dtype=np.int32), np.zeros(around.shape, dtype=np.int32)
    for k in np.ndindex(around.shape):
        a = around[k]
        if not np.isfinite(a):
            continue
        first = max(0, int(math.ceil((a - half_width - t0) * fs)))
        last = min(nt - 1, int(math.floor((a + half_width - t0) * fs)))
        if first <= last:
            lo[k], hi[k] = first, last + 1
    return lo, hi


# ---- tests/trace_pick_sim.cpp ----

def write_sim_input(path, data, lo, hi, mode, frac, guard):
    """int64[8] header (ntrace, nt, ncomp, dtype, mode, guard, the bits of frac, 0), int32 lo[ntrace],
    int32 hi[ntrace], the data [ntrace][nt][ncomp] in their dtype."""
    data = np.asarray(data)
    cplx = np.iscomplexobj(data)
    f32 = data.dtype in (np.float32, np.complex64)
    nt = data.shape[-1]
    hdr = np.array([data.size // nt, nt, 2 if cplx else 1, int(f32), mode, guard,
                    np.array([frac], dtype=np.float64).view(np.int64)[0], 0], dtype=np.int64)
    with open(path, "wb") as f:
        f.write(hdr.tobytes())
        f.write(np.ascontiguousarray(lo, dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(hi, dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(data).tobytes())


def read_sim_output(path, ntrace):
    """The program's output: pos, amp, amp2 float64 [ntrace] each, then idx, idx2, flags int32."""
    with open(path, "rb") as f:
        d = np.frombuffer(f.read(24 * ntrace), dtype=np.float64).reshape(3, ntrace)
        i = np.frombuffer(f.read(12 * ntrace), dtype=np.int32).reshape(3, ntrace)
    return d[0].copy(), d[1].copy(), i[0].copy(), d[2].copy(), i[1].copy(), i[2].copy()
