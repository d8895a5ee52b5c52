"""Least-squares imaging from resident fields (alifmm_tfm_f64, alifmm_tfm_lsq) on the TFM workload of
tools/tfm_bench.py and tools/tfm_model_bench.py (GPU box): the 4096^2 weld-like grid, 64 elements
on the top row, their fields computed by travel(copy_out=False) and left on the device, nt = 4096,
complex data; fs is chosen so that every delay is in range.  Per window (the centred 1024^2 window
and the whole 4096^2 grid): kernel ms of the float64 and the float32 TFM on the same noise data
(best of the repeats, HIP events in the library), the chunk sweep of both ("tfm_chunk" 4, 8, 16,
32), device ms per CGLS iteration of alifmm_tfm_lsq (the difference of solves of 1 and of
1 + --iters iterations, damp > 0, tol 0), and wall ms per iteration of the same CGLS done the only
way the library allowed before alifmm_tfm_lsq: Context.tfm on the float32 cast of the residual,
Context.tfm_model, and the vector updates in numpy.  With --parent-pkg DIR the host route runs in
a child process on the package directory DIR of a built checkout of the commit before
alifmm_tfm_lsq (its _alifmm.py and lib/libalifmm.so), in the same session; without it, on this
build (the two calls it uses are unchanged).
python tools/tfm_lsq_bench.py [--n 4096] [--elements 64] [--nt 4096] [--repeats 3] [--iters 2]
                              [--parent-pkg DIR] [--no-full] [--out FILE]
-> one JSON line, also written to FILE (default profiles/tfm_lsq_bench.json)"""
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
import _alifmm  # noqa: E402
import workloads as W  # noqa: E402

DAMP = 0.64  # 1e-2 of sqrt(64 x 64), the order of |A|_2


def setup(n, ne, nt):
    ctx = _alifmm.Context(0)
    vt = W.default_table()
    ctx.set_model(*W.weldlike_model(n), vt, vt, W.weldlike_dnx())
    sx, sz = W.c4_sources(ne, n)
    t = time.perf_counter()
    ctx.travel(sx, sz, copy_out=False)
    travel_s = time.perf_counter() - t
    tmax = max(ctx.get_field(0, 1).max(), ctx.get_field(ne - 1, 1).max())
    return ctx, (nt - 2) / (2.0 * tmax), travel_s


def windows(n, full):
    w = min(1024, n)
    o = (n - w) // 2
    wins = [("window_%d" % w, (o, o, w, w))]
    if full and n > w:
        wins.append(("full_%d" % n, (0, 0, n, n)))
    return wins


def host_route(ctx, slots, d, fs, window, iters):
    """Wall ms per iteration of CGLS (damp only) through Context.tfm on the float32 cast of the
    residual, Context.tfm_model and numpy; the start (Aᵀ d) is not counted."""
    d2 = DAMP * DAMP
    r = d.copy()
    s = ctx.tfm(slots, slots, r.astype(np.complex64), fs, window=window)
    p = s.copy()
    x = np.zeros_like(s)
    gamma = float(np.vdot(s, s).real)
    t = time.perf_counter()
    for _ in range(iters):
        q = ctx.tfm_model(slots, slots, p, fs, d.shape[2], window=window)
        qq = float(np.vdot(q, q).real) + d2 * float(np.vdot(p, p).real)
        alpha = gamma / qq
        x += alpha * p
        r -= alpha * q
        s = ctx.tfm(slots, slots, r.astype(np.complex64), fs, window=window) - d2 * x
        new = float(np.vdot(s, s).real)
        p = s + (new / gamma) * p
        gamma = new
    return 1e3 * (time.perf_counter() - t) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--elements", type=int, default=64)
    ap.add_argument("--nt", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--parent-pkg", default=None, help="built package directory of the commit before alifmm_tfm_lsq")
    ap.add_argument("--host-route-only", action="store_true", help="(the child process of --parent-pkg)")
    ap.add_argument("--no-full", action="store_true", help="skip the whole grid")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tfm_lsq_bench.json"))
    a = ap.parse_args()
    n, ne, nt = a.n, a.elements, a.nt
    wins = windows(n, not a.no_full)
    if a.parent_pkg and not a.host_route_only:
        # a fresh process on the other library, before this one opens the GPU
        env = dict(os.environ, ALIFMM_BENCH_PKG=os.path.abspath(a.parent_pkg))
        cmd = [sys.executable, os.path.abspath(__file__), "--host-route-only", "--n", str(n), "--elements", str(ne),
               "--nt", str(nt), "--iters", str(a.iters), "--out", ""] + (["--no-full"] if a.no_full else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, check=True)
        host = json.loads(r.stdout.strip().splitlines()[-1])
    ctx, fs, travel_s = setup(n, ne, nt)
    slots = list(range(ne))
    d = np.random.default_rng(5).standard_normal((ne, ne, nt, 2)).view(np.complex128)[..., 0]
    if a.host_route_only or not a.parent_pkg:
        host = {"library": "the commit before alifmm_tfm_lsq" if os.environ.get("ALIFMM_BENCH_PKG") else "this build"}
        for name, win in wins:
            host_route(ctx, slots, d, fs, (win[0], win[1], 64, 64), 1)  # warm-up
            host[name] = round(host_route(ctx, slots, d, fs, win, a.iters), 1)
        if a.host_route_only:
            print(json.dumps(host), flush=True)
            ctx.close()
            return
    out = {"n": n, "elements": ne, "nt": nt, "fs_hz": fs, "travel_s": round(travel_s, 3),
           "data_MB_f64": round(ne * ne * nt * 16 / 1e6, 1), "n_cu": int(ctx.get_option("n_cu")), "damp": DAMP,
           "host_route_wall_ms_per_iter": host}
    d32 = d.astype(np.complex64)

    def tfm_ms(data, window, precision, repeats):
        best = None
        for _ in range(repeats):
            ctx.tfm(slots, slots, data, fs, window=window, precision=precision)
            ms = ctx.get_option("tfm_kernel_ms")
            best = ms if best is None else min(best, ms)
        return round(best, 3)

    tfm_ms(d, (0, 0, 64, 64), "f64", 1)  # warm-up: code objects, buffers
    tfm_ms(d32, (0, 0, 64, 64), "f32", 1)
    for name, win in wins:
        rec = {}
        big = win[2] > 1024
        for chunk in (4, 8, 16, 32):
            ctx.set_option("tfm_chunk", chunk)
            rep = 1 if big and chunk != 8 else a.repeats
            rec["chunk%d" % chunk] = {"f64_kernel_ms": tfm_ms(d, win, "f64", rep), "f32_kernel_ms": tfm_ms(d32, win, "f32", rep)}
        ctx.set_option("tfm_chunk", 8)
        ctx.tfm(slots, slots, d, fs, window=win, precision="f64")
        rec["upload_ms_f64"] = round(ctx.get_option("tfm_upload_ms"), 1)
        # the solve: 1 and 1 + iters iterations, the difference is the iterations' device time
        ks = {}
        for k in (1, 1 + a.iters):
            best = None
            for _ in range(1 if big else a.repeats):
                t = time.perf_counter()
                x, info = ctx.tfm_lsq(slots, slots, d, fs, window=win, damp=DAMP, max_iter=k, tol=0.0)
                wall = 1e3 * (time.perf_counter() - t)
                ms = ctx.get_option("tfm_lsq_kernel_ms")
                if best is None or ms < best[0]:
                    best = (ms, wall)
            assert info["iterations"] == k and info["reason"] == "max_iter"
            ks[k] = best
        per = (ks[1 + a.iters][0] - ks[1][0]) / a.iters
        rec["lsq"] = {"kernel_ms_1_iter": round(ks[1][0], 2), "kernel_ms_%d_iters" % (1 + a.iters): round(ks[1 + a.iters][0], 2),
                      "device_ms_per_iter": round(per, 2), "upload_ms": round(ctx.get_option("tfm_lsq_upload_ms"), 1),
                      "wall_ms_%d_iters" % (1 + a.iters): round(ks[1 + a.iters][1], 1),
                      "model_slabs_used": int(ctx.get_option("tfm_model_slabs_used")),
                      "res_norm_over_rhs_norm": info["res_norm"] / info["rhs_norm"]}
        rec["host_over_device_per_iter"] = round(host[name] / per, 2)
        out[name] = rec
    ctx.close()
    out["notes"] = ("kernel ms: HIP events in the library, best of %d (the whole grid: chunk 8 only, the rest once); "
                    "device_ms_per_iter: (device time of a solve of %d iterations - of 1) / %d, each solve from the upload "
                    "of the data on; host route: wall clock of an iteration with its two 268 MB transfers per product"
                    % (a.repeats, 1 + a.iters, a.iters))
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
