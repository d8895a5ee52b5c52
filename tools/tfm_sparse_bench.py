"""Sparsity-regularised imaging (alifmm_tfm_sparse) on the TFM workload of tools/tfm_lsq_bench.py and
tools/trace_fir_bench.py (GPU box): the 4096^2 weld-like grid, 64 elements on the top row, their
fields computed by travel(copy_out=False) and left on the device, nt = 4096, complex data; fs is
chosen so that every delay is in range.  Per window (the centred 1024^2 window and the whole 4096^2
grid), without a pulse and with the 64-tap complex pulse of trace_fir_bench.py:
  - device ms per accepted FISTA iteration of alifmm_tfm_sparse (the difference of solves of 1 and
    of 1 + --iters iterations, tol 0, lam = 0.1 lam_max, L given as four times a short power
    estimate so that no trial is rejected; the backtracks are reported and must be 0);
  - the yardstick: device ms per CGLS iteration of alifmm_tfm_lsq / alifmm_tfm_lsq_pulse measured the
    same way, and the ratio of the two.  Both iterations run the same two products (and the same
    two FIR passes), so the difference is the vector passes;
  - the bytes the vector passes of either iteration move, from the shapes (data-space vectors only:
    FISTA's trial pass reads B x+ and d, its momentum pass reads B x+, B x and d and writes r, six
    vectors; CGLS's step reads q, then reads r and q and writes r, four), and what they cost at the
    6.3 TB/s a streaming kernel reaches on this GPU;
  - wall ms per iteration of the same FISTA done the only way the library allowed before
    alifmm_tfm_sparse: Context.tfm_model, Context.trace_fir, Context.tfm(precision="f64"), the prox
    and the updates in numpy (L given: no rejected trial).
With --parent-pkg DIR the yardstick and the host route run in a child process on the package
directory DIR of a built checkout of the commit before alifmm_tfm_sparse (its _alifmm.py and
lib/libalifmm.so), in the same session; without it, on this build (the calls they use are unchanged).
python tools/tfm_sparse_bench.py [--n 4096] [--elements 64] [--nt 4096] [--taps 64] [--repeats 3] [--iters 2]
                                 [--parent-pkg DIR] [--no-full] [--out FILE]
-> one JSON line, also written to FILE (default profiles/tfm_sparse_bench.json)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("ALIFMM_BENCH_PKG") or os.path.join(REPO, "ali-fmm-and-ray-tracing_amd")  # (the child of --parent-pkg)
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(REPO, "tests"))
import _alifmm  # noqa: E402,F401

from tfm_lsq_bench import DAMP, setup, windows  # noqa: E402  (the same workload)
from trace_fir_bench import lsq_per_iter, pulse  # noqa: E402

STREAM_TBPS = 6.3  # what a streaming kernel reaches of the HBM's 8 TB/s


def host_route(ctx, slots, d, fs, window, h, origin, lam_rel, iters):
    """Wall ms per iteration of FISTA (damp only; L four times two rounds of the power method, so no
    trial is rejected) through Context.tfm_model, Context.trace_fir, Context.tfm(precision="f64") and
    numpy; the start (Aᵀ Pᵀ d and the estimate of L) is not counted."""
    d2 = DAMP * DAMP
    nt = d.shape[2]

    def fwd(v):
        q = ctx.tfm_model(slots, slots, v, fs, nt, window=window)
        return q if h is None else ctx.trace_fir(q, h, origin)

    def adj(r):
        return ctx.tfm(slots, slots, r if h is None else ctx.trace_fir(r, h, origin, transpose=True), fs, window=window,
                       precision="f64")

    g0 = adj(d)
    lam = lam_rel * float(np.abs(g0).max())
    v, lip = g0 / np.linalg.norm(g0), 0.0
    for _ in range(2):
        w = adj(fwd(v)) + d2 * v
        lip = float(np.linalg.norm(w))
        v = w / lip
    lip *= 4.0
    x = np.zeros_like(g0)
    y, bx, g, theta = x, np.zeros_like(d), -g0, 1.0
    t = time.perf_counter()
    for _ in range(iters):
        z = y - g / lip
        m = np.abs(z)
        xn = z * (np.maximum(m - lam / lip, 0.0) / np.where(m > 0, m, 1.0))
        bxn = fwd(xn)
        # (the accept test's sums: the cost of forming them belongs to the route)
        rn = bxn - d
        fn = 0.5 * float(np.vdot(rn, rn).real) + 0.5 * d2 * float(np.vdot(xn, xn).real)
        dy = xn - y
        q = float(np.vdot(g, dy).real) + 0.5 * lip * float(np.vdot(dy, dy).real)
        theta1 = (1 + np.sqrt(1 + 4 * theta * theta)) / 2
        beta = (theta - 1) / theta1
        theta = theta1
        y = xn + beta * (xn - x)
        r = bxn + beta * (bxn - bx) - d
        x, bx = xn, bxn
        g = adj(r) + d2 * y
    assert np.isfinite(fn) and np.isfinite(q)
    return 1e3 * (time.perf_counter() - t) / iters


def sparse_per_iter(ctx, slots, d, fs, win, iters, repeats, **pulse_kw):
    """Device ms per accepted iteration: (a solve of 1 + iters iterations - a solve of 1) / iters,
    best of repeats, and the L they ran with."""
    ctx.tfm_sparse(slots, slots, d, fs, window=win, damp=DAMP, lam_rel=0.1, lipschitz=0.0, power_iters=3, max_iter=1, tol=0.0,
                   **pulse_kw)
    lip = 4.0 * ctx.get_option("tfm_sparse_l0")
    ks = {}
    for k in (1, 1 + iters):
        best = None
        for _ in range(repeats):
            x, info = ctx.tfm_sparse(slots, slots, d, fs, window=win, damp=DAMP, lam_rel=0.1, lipschitz=lip, max_iter=k,
                                     tol=0.0, **pulse_kw)
            ms = ctx.get_option("tfm_sparse_kernel_ms")
            best = ms if best is None else min(best, ms)
            assert info["iterations"] == k and info["reason"] == "max_iter" and info["backtracks"] == 0, info
        ks[k] = best
    return {"kernel_ms_1_iter": round(ks[1], 2), "kernel_ms_%d_iters" % (1 + iters): round(ks[1 + iters], 2),
            "device_ms_per_iter": round((ks[1 + iters] - ks[1]) / iters, 2), "lipschitz": lip, "nnz": info["nnz"],
            "upload_ms": round(ctx.get_option("tfm_sparse_upload_ms"), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--elements", type=int, default=64)
    ap.add_argument("--nt", type=int, default=4096)
    ap.add_argument("--taps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--parent-pkg", default=None, help="built package directory of the commit before alifmm_tfm_sparse")
    ap.add_argument("--yardstick-only", action="store_true", help="(the child process of --parent-pkg)")
    ap.add_argument("--no-full", action="store_true", help="skip the whole grid")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tfm_sparse_bench.json"))
    a = ap.parse_args()
    n, ne, nt = a.n, a.elements, a.nt
    wins = windows(n, not a.no_full)
    h, origin = pulse(a.taps, True), a.taps // 2
    cases = [("no_pulse", None, {}), ("pulse_%d" % a.taps, h, dict(pulse=h, pulse_origin=origin))]
    slots = list(range(ne))
    d = np.random.default_rng(5).standard_normal((ne, ne, nt, 2)).view(np.complex128)[..., 0]

    def yardstick(ctx, fs):
        y = {"library": "the commit before alifmm_tfm_sparse" if os.environ.get("ALIFMM_BENCH_PKG") else "this build"}
        ctx.tfm_lsq(slots, slots, d, fs, window=(0, 0, 64, 64), damp=DAMP, max_iter=1, pulse=h, pulse_origin=origin)  # warm-up
        for name, win in wins:
            big = win[2] > 1024
            y[name] = {}
            for cname, hh, kw in cases:
                rec = {"cgls": lsq_per_iter(ctx, slots, d, fs, win, a.iters, 1 if big else a.repeats, **kw)}
                host_route(ctx, slots, d, fs, (win[0], win[1], 64, 64), hh, origin, 0.1, 1)  # warm-up
                rec["host_route_wall_ms_per_iter"] = round(
                    host_route(ctx, slots, d, fs, win, hh, origin, 0.1, 1 if big else a.iters), 1)
                y[name][cname] = rec
        return y

    if a.yardstick_only:
        ctx, fs, travel_s = setup(n, ne, nt)
        print(json.dumps(yardstick(ctx, fs)), flush=True)
        ctx.close()
        return
    yard = None
    if a.parent_pkg:
        # a fresh process on the other library, before this one opens the GPU
        env = dict(os.environ, ALIFMM_BENCH_PKG=os.path.abspath(a.parent_pkg))
        cmd = [sys.executable, os.path.abspath(__file__), "--yardstick-only", "--n", str(n), "--elements", str(ne), "--nt",
               str(nt), "--taps", str(a.taps), "--iters", str(a.iters), "--repeats", str(a.repeats), "--out", ""]
        r = subprocess.run(cmd + (["--no-full"] if a.no_full else []), env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("the yardstick failed: %s" % r.stderr[-2000:])
        yard = json.loads(r.stdout.strip().splitlines()[-1])
    ctx, fs, travel_s = setup(n, ne, nt)
    out = {"n": n, "elements": ne, "nt": nt, "taps": a.taps, "fs_hz": fs, "travel_s": round(travel_s, 3),
           "data_MB_f64": round(ne * ne * nt * 16 / 1e6, 1), "n_cu": int(ctx.get_option("n_cu")), "damp": DAMP,
           "lam_rel": 0.1}
    ctx.tfm_sparse(slots, slots, d, fs, window=(0, 0, 64, 64), damp=DAMP, lam_rel=0.1, max_iter=1, pulse=h,
                   pulse_origin=origin)  # warm-up: code objects
    for name, win in wins:
        big = win[2] > 1024
        out[name] = {}
        for cname, hh, kw in cases:
            # the two iterations side by side: the same products, so the difference is the vector passes
            rec = sparse_per_iter(ctx, slots, d, fs, win, a.iters, 1 if big else a.repeats, **kw)
            own = lsq_per_iter(ctx, slots, d, fs, win, a.iters, 1 if big else a.repeats, **kw)
            out[name][cname] = {"fista": rec, "cgls_this_build": own}
    if yard is None:
        yard = yardstick(ctx, fs)
    ctx.close()
    out["yardstick_library"] = yard["library"]
    vec_bytes = ne * ne * nt * 16
    for name, win in wins:
        for cname, hh, kw in cases:
            rec = out[name][cname]
            rec.update(yard[name][cname])
            f, c, o = (rec[k]["device_ms_per_iter"] for k in ("fista", "cgls", "cgls_this_build"))
            rec["fista_over_cgls_per_iter"] = round(f / c, 3)
            rec["fista_over_cgls_this_build_per_iter"] = round(f / o, 3)
            rec["fista_minus_cgls_this_build_ms"] = round(f - o, 2)
            rec["host_over_device_per_iter"] = round(rec["host_route_wall_ms_per_iter"] / f, 1)
    out["vector_passes"] = {"fista_data_vectors_moved": 6, "cgls_data_vectors_moved": 4,
                            "fista_ms_at_%.1f_TBps" % STREAM_TBPS: round(6 * vec_bytes / (STREAM_TBPS * 1e9), 3),
                            "cgls_ms_at_%.1f_TBps" % STREAM_TBPS: round(4 * vec_bytes / (STREAM_TBPS * 1e9), 3)}
    out["notes"] = ("device_ms_per_iter: (device time of a solve of %d iterations - of 1) / %d, HIP events in the library, "
                    "best of %d (the whole grid: once); the vector kernels' own device time is not measured separately: "
                    "fista_minus_cgls_this_build_ms is the difference of the two iterations measured back to back in one process, which share their products; cgls: the yardstick's, in its own process before this one; host route: "
                    "wall clock of an iteration with its 268 MB transfers per product and per FIR pass"
                    % (1 + a.iters, a.iters, a.repeats))
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
