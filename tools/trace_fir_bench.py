"""The trace FIR (alifmm_trace_fir) and pulse-aware least-squares imaging (alifmm_tfm_lsq_pulse) on the
TFM workload of tools/tfm_lsq_bench.py (GPU box): the 4096^2 weld-like grid, 64 elements on the top
row, their fields computed by travel(copy_out=False) and left on the device, nt = 4096, complex
data; fs is chosen so that every delay is in range.
  - the FIR kernel alone on the 64 x 64 traces of 4096 complex samples: kernel ms (best of the
    repeats, HIP events in the library) forward and transposed, at 64 real and at 64 complex taps,
    with the float64 operations (2 per real product-and-add and component, 8 per complex one) and
    the bytes moved (one read and one write of the traces) that go with them;
  - per window (the centred 1024^2 window and the whole 4096^2 grid): device ms per CGLS iteration
    of the pulse-aware solve at 64 complex taps and of the pulse-less solve (the difference of solves
    of 1 and of 1 + --iters iterations, damp > 0, tol 0);
  - the yardstick, the build before alifmm_tfm_lsq_pulse: device ms per iteration of its pulse-less
    alifmm_tfm_lsq, and wall ms per iteration of the only pulse-aware route it allows:
    Context.tfm_model, a numpy FFT convolution with the pulse, the numpy FFT correlation of the
    residual, Context.tfm(precision="f64") on it, and the vector updates in numpy.
With --parent-pkg DIR the yardstick runs in a child process on the package directory DIR of a built
checkout of the commit before alifmm_tfm_lsq_pulse (its _alifmm.py and lib/libalifmm.so), in the
same session; without it, on this build (the calls it uses are unchanged).
python tools/trace_fir_bench.py [--n 4096] [--elements 64] [--nt 4096] [--taps 64] [--repeats 3] [--iters 2]
                                [--parent-pkg DIR] [--no-full] [--out FILE]
-> one JSON line, also written to FILE (default profiles/trace_fir_bench.json)"""
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

from tfm_lsq_bench import DAMP, setup, windows  # noqa: E402  (the same workload)


def pulse(ntap, cplx):
    """A Gaussian-windowed tone of 6 cycles over the taps, time zero at the middle tap."""
    k = np.arange(ntap) - (ntap - 1) / 2
    env = np.exp(-0.5 * (k / (ntap / 6.0)) ** 2)
    phi = 2 * np.pi * 6 * k / ntap
    return env * np.exp(1j * phi) if cplx else env * np.cos(phi)


def fft_fir(x, h, origin, transpose):
    """trace_fir() by numpy's FFT in float64, to rounding."""
    nt = x.shape[-1]
    n = nt + len(h) - 1
    if transpose:  # z[t] = sum_j conj(h[j]) y[t + j - origin]: the convolution with the reversed conjugate
        h, origin = np.conj(h[::-1]), len(h) - 1 - origin
    full = np.fft.ifft(np.fft.fft(x, n, axis=-1) * np.fft.fft(h.astype(np.complex128), n), axis=-1)
    return np.ascontiguousarray(full[..., origin:origin + nt])


def host_route(ctx, slots, d, fs, window, h, origin, iters):
    """Wall ms per iteration of CGLS (damp only) on P A through Context.tfm_model, numpy's FFT,
    Context.tfm(precision="f64") and numpy; the start (Aᵀ Pᵀ d) is not counted."""
    d2 = DAMP * DAMP
    r = d.copy()
    s = ctx.tfm(slots, slots, fft_fir(r, h, origin, True), fs, window=window, precision="f64")
    p = s.copy()
    x = np.zeros_like(s)
    gamma = float(np.vdot(s, s).real)
    t = time.perf_counter()
    for _ in range(iters):
        q = fft_fir(ctx.tfm_model(slots, slots, p, fs, d.shape[2], window=window), h, origin, False)
        qq = float(np.vdot(q, q).real) + d2 * float(np.vdot(p, p).real)
        alpha = gamma / qq
        x += alpha * p
        r -= alpha * q
        s = ctx.tfm(slots, slots, fft_fir(r, h, origin, True), fs, window=window, precision="f64") - d2 * x
        new = float(np.vdot(s, s).real)
        p = s + (new / gamma) * p
        gamma = new
    return 1e3 * (time.perf_counter() - t) / iters


def lsq_per_iter(ctx, slots, d, fs, win, iters, repeats, **pulse_kw):
    """Device ms per iteration: (a solve of 1 + iters iterations - a solve of 1) / iters, best of repeats."""
    ks = {}
    for k in (1, 1 + iters):
        best = None
        for _ in range(repeats):
            x, info = ctx.tfm_lsq(slots, slots, d, fs, window=win, damp=DAMP, max_iter=k, tol=0.0, **pulse_kw)
            ms = ctx.get_option("tfm_lsq_kernel_ms")
            best = ms if best is None else min(best, ms)
        assert info["iterations"] == k and info["reason"] == "max_iter"
        ks[k] = best
    return {"kernel_ms_1_iter": round(ks[1], 2), "kernel_ms_%d_iters" % (1 + iters): round(ks[1 + iters], 2),
            "device_ms_per_iter": round((ks[1 + iters] - ks[1]) / iters, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--elements", type=int, default=64)
    ap.add_argument("--nt", type=int, default=4096)
    ap.add_argument("--taps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--parent-pkg", default=None, help="built package directory of the commit before alifmm_tfm_lsq_pulse")
    ap.add_argument("--yardstick-only", action="store_true", help="(the child process of --parent-pkg)")
    ap.add_argument("--no-full", action="store_true", help="skip the whole grid")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trace_fir_bench.json"))
    a = ap.parse_args()
    n, ne, nt = a.n, a.elements, a.nt
    wins = windows(n, not a.no_full)
    h, origin = pulse(a.taps, True), a.taps // 2
    if a.parent_pkg and not a.yardstick_only:
        # a fresh process on the other library, before this one opens the GPU
        env = dict(os.environ, ALIFMM_BENCH_PKG=os.path.abspath(a.parent_pkg))
        cmd = [sys.executable, os.path.abspath(__file__), "--yardstick-only", "--n", str(n), "--elements", str(ne), "--nt",
               str(nt), "--taps", str(a.taps), "--iters", str(a.iters), "--repeats", str(a.repeats), "--out", ""]
        r = subprocess.run(cmd + (["--no-full"] if a.no_full else []), env=env, capture_output=True, text=True, check=True)
        yard = json.loads(r.stdout.strip().splitlines()[-1])
    ctx, fs, travel_s = setup(n, ne, nt)
    slots = list(range(ne))
    d = np.random.default_rng(5).standard_normal((ne, ne, nt, 2)).view(np.complex128)[..., 0]
    ctx.tfm_lsq(slots, slots, d, fs, window=(0, 0, 64, 64), damp=DAMP, max_iter=1, tol=0.0)  # warm-up: code objects, buffers
    if a.yardstick_only or not a.parent_pkg:
        yard = {"library": "the commit before alifmm_tfm_lsq_pulse" if os.environ.get("ALIFMM_BENCH_PKG") else "this build",
                "lsq_device_ms_per_iter": {}, "host_route_wall_ms_per_iter": {}}
        for name, win in wins:
            big = win[2] > 1024
            yard["lsq_device_ms_per_iter"][name] = lsq_per_iter(ctx, slots, d, fs, win, a.iters, 1 if big else a.repeats)
            host_route(ctx, slots, d, fs, (win[0], win[1], 64, 64), h, origin, 1)  # warm-up
            yard["host_route_wall_ms_per_iter"][name] = round(host_route(ctx, slots, d, fs, win, h, origin, a.iters), 1)
        if a.yardstick_only:
            print(json.dumps(yard), flush=True)
            ctx.close()
            return
    out = {"n": n, "elements": ne, "nt": nt, "taps": a.taps, "fs_hz": fs, "travel_s": round(travel_s, 3),
           "data_MB_f64": round(ne * ne * nt * 16 / 1e6, 1), "n_cu": int(ctx.get_option("n_cu")), "damp": DAMP,
           "trace_fir_tile": int(ctx.get_option("trace_fir_tile")), "yardstick": yard}
    # the kernel alone
    fir = {}
    for kind, taps, flops in (("real_taps", pulse(a.taps, False), 4), ("complex_taps", h, 8)):
        for transpose in (False, True):
            best = None
            for _ in range(a.repeats + 1):  # (the first call loads the code object)
                y = ctx.trace_fir(d, taps, origin=origin, transpose=transpose)
                ms = ctx.get_option("trace_fir_kernel_ms")
                best = ms if best is None else min(best, ms)
            ops = ne * ne * nt * a.taps * flops
            fir["%s_%s" % (kind, "transposed" if transpose else "forward")] = {
                "kernel_ms": round(best, 3), "f64_gflop": round(ops / 1e9, 2), "f64_tflops": round(ops / best / 1e9, 2),
                "traffic_GBps": round(2 * d.nbytes / best / 1e6, 1)}
        ref = fft_fir(d[:2, :2], taps.astype(np.complex128), origin, True)  # (the last call: transposed)
        fir[kind + "_max_dev_from_fft"] = float(np.abs(y[:2, :2] - ref).max() / np.abs(ref).max())
    out["trace_fir_kernel"] = fir
    for name, win in wins:
        big = win[2] > 1024
        rep = 1 if big else a.repeats
        rec = {"pulse_aware": lsq_per_iter(ctx, slots, d, fs, win, a.iters, rep, pulse=h, pulse_origin=origin),
               "pulse_less": lsq_per_iter(ctx, slots, d, fs, win, a.iters, rep),
               "model_slabs_used": int(ctx.get_option("tfm_model_slabs_used"))}
        per = rec["pulse_aware"]["device_ms_per_iter"]
        rec["pulse_aware_over_yardstick_pulse_less"] = round(per / yard["lsq_device_ms_per_iter"][name]["device_ms_per_iter"], 3)
        rec["pulse_aware_over_pulse_less_this_build"] = round(per / rec["pulse_less"]["device_ms_per_iter"], 3)
        rec["yardstick_host_route_over_pulse_aware"] = round(yard["host_route_wall_ms_per_iter"][name] / per, 2)
        out[name] = rec
    ctx.close()
    out["notes"] = ("kernel ms: HIP events in the library, best of %d; device_ms_per_iter: (device time of a solve of %d "
                    "iterations - of 1) / %d, each solve from the upload of the data on (the whole grid: once); host route: "
                    "wall clock of an iteration with its 268 MB transfers and FFTs per product; f64_tflops and "
                    "traffic_GBps: the operations and bytes of the algorithm over the kernel's time"
                    % (a.repeats, 1 + a.iters, a.iters))
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
