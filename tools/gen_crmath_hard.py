#!/usr/bin/env python3
"""One-off generator of tests/golden/crmath_hard.npz: arguments on which csrc/cr_math.h's fast paths
cannot decide the rounding.

For each function (atan, sin, cos, tan) and each of its two ranges, 2^21 seeded arguments are
evaluated with mpmath (tests/crmath_cases.py, 200 bits) and the 1024 are kept whose exact value lies
nearest, relative to the value, to a midpoint between adjacent doubles.  The fixture holds arguments
only (float64, 8 x 1024); expected values are recomputed by the tests.  The 1024th distance of every
scan must be below 2^-63 (the fast paths' tightest error bound); a scan that misses it needs more
arguments (--log2n), never a looser bound.  A few minutes on a handful of cores.

    python tools/gen_crmath_hard.py [--jobs 8] [--log2n 21]
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import crmath_cases as C  # noqa: E402

KEEP = 1024
RANGES = {  # name -> (seed, draw(rng, n))
    "4pi": (11, lambda r, n: (r.random(n) * 2 - 1) * (4 * np.pi)),
    "16k": (12, lambda r, n: (r.random(n) * 2 - 1) * 16383.9),
    "log": (13, lambda r, n: np.exp2(r.random(n) * 92 - 30) * r.choice([-1.0, 1.0], n)),
    "02": (14, lambda r, n: r.random(n) * 2),
}


def _scan(job):
    kind, x = job
    if kind == "atan":
        return np.array([[C._mid_dist(C._exact("atan", xi)[0])] for xi in x.tolist()])
    return np.array([[C._mid_dist(v) for v in C._exact("trig", xi)] for xi in x.tolist()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--out", default=C.HARD_FILE)
    a = ap.parse_args()
    n = 1 << a.log2n
    out = {}
    with multiprocessing.Pool(a.jobs) as pool:
        for rname, (seed, draw) in RANGES.items():
            kind = "atan" if rname in ("log", "02") else "trig"
            x = draw(np.random.default_rng(seed), n)
            x = x[(x != 0) & np.isfinite(x)]
            d = np.vstack(pool.map(_scan, [(kind, c) for c in np.array_split(x, 64 * a.jobs)]))
            for col, f in enumerate(("atan",) if kind == "atan" else ("sin", "cos", "tan")):
                order = np.argsort(d[:, col], kind="stable")[:KEEP]
                worst = d[order[-1], col]
                print("%s_%s: %d arguments, 1024th distance 2^%.2f" % (f, rname, len(x), np.log2(worst)), flush=True)
                if not worst < C.HARD_BOUND:
                    sys.exit("%s_%s: the 1024th distance is not below 2^-63: enlarge the scan (--log2n)" % (f, rname))
                out["%s_%s" % (f, rname)] = x[np.sort(order)]
    np.savez(a.out, **out)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
