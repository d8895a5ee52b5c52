"""The spectral trace filter (alifmm_trace_spectral) as the RF front end of the TFM workload of
tools/tfm_lsq_bench.py (GPU box): 64 x 64 real float32 traces of 4096 samples made analytic.
  - at nfft 4096 and 8192, without a response and with a band-pass: kernel ms (HIP events in the
    library), upload and download ms (host clock in the library) and the whole call's wall ms, best
    of the repeats, with the deviation of the last result from the numpy route;
  - in the same session, the numpy route on this host's CPU: np.fft.fft in float64 at the same nfft,
    times the mask and the response, np.fft.ifft, cut to nt, cast to complex64 (wall ms, best);
  - tfm_kernel_ms of the centred 1024^2 window on the analytic data, on the 4096^2 weld-like grid
    with the elements' fields resident.
python tools/trace_fft_bench.py [--n 4096] [--elements 64] [--nt 4096] [--repeats 3] [--out FILE]
-> one JSON line, also written to FILE (default profiles/trace_fft_bench.json)"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ali-fmm-and-ray-tracing_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import _alifmm  # noqa: E402

from tfm_lsq_bench import setup, windows  # noqa: E402  (the same workload)


def numpy_route(x, nfft, h):
    """scipy.signal.hilbert's definition by numpy's FFT in float64, with the response."""
    n = nfft
    m = np.zeros(n)
    m[0] = m[n // 2] = 1.0
    m[1:n // 2] = 2.0
    X = np.fft.fft(x.astype(np.float64), n=n, axis=-1) * (m if h is None else m * h)
    return np.fft.ifft(X, axis=-1)[..., :x.shape[-1]].astype(np.complex64)


def best_of(f, repeats):
    best, res = None, None
    for _ in range(repeats):
        t = time.perf_counter()
        res = f()
        ms = 1e3 * (time.perf_counter() - t)
        best = ms if best is None else min(best, ms)
    return best, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--elements", type=int, default=64)
    ap.add_argument("--nt", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trace_fft_bench.json"))
    a = ap.parse_args()
    n, ne, nt = a.n, a.elements, a.nt
    ctx, fs, travel_s = setup(n, ne, nt)
    slots = list(range(ne))
    rf = np.random.default_rng(5).standard_normal((ne, ne, nt)).astype(np.float32)
    ctx.trace_spectral(rf[:1], analytic=True)  # warm-up: the code object
    out = {"n": n, "elements": ne, "nt": nt, "fs_hz": fs, "travel_s": round(travel_s, 3),
           "rf_MB_f32": round(rf.nbytes / 1e6, 1), "analytic_MB_c64": round(2 * rf.nbytes / 1e6, 1),
           "n_cu": int(ctx.get_option("n_cu")), "trace_fft_grid": int(ctx.get_option("trace_fft_grid")),
           "host_cpus": len(os.sched_getaffinity(0))}
    for nfft in (nt, 2 * nt):
        for name, h in (("analytic", None), ("analytic_bandpass", _alifmm.bandpass_response(nfft, fs, 0.1 * fs, 0.3 * fs))):
            rec = {}
            for _ in range(a.repeats + 1):  # (the first call grows the buffers)
                t = time.perf_counter()
                y = ctx.trace_spectral(rf, response=h, analytic=True, nfft=nfft)
                got = {"call_ms": 1e3 * (time.perf_counter() - t), "kernel_ms": ctx.get_option("trace_fft_kernel_ms"),
                       "upload_ms": ctx.get_option("trace_fft_upload_ms"), "download_ms": ctx.get_option("trace_fft_download_ms")}
                rec = {k: min(v, rec.get(k, v)) for k, v in got.items()}
            np_ms, ref = best_of(lambda: numpy_route(rf, nfft, h), a.repeats)
            rec = {k: round(v, 3) for k, v in rec.items()}
            rec["numpy_route_ms"] = round(np_ms, 1)
            rec["numpy_over_call"] = round(np_ms / rec["call_ms"], 2)
            rec["numpy_over_kernel"] = round(np_ms / rec["kernel_ms"], 1)
            rec["max_dev_from_numpy"] = float(np.abs(y - ref).max() / np.abs(ref).max())
            # the algorithm's operations (10 flops a butterfly, two transforms) and the traffic of the kernel
            lg = nfft.bit_length() - 1
            rec["f64_tflops"] = round(ne * ne * 2 * 10 * (nfft // 2) * lg / rec["kernel_ms"] / 1e9, 2)
            rec["traffic_GBps"] = round(3 * rf.nbytes / rec["kernel_ms"] / 1e6, 1)
            out["nfft_%d_%s" % (nfft, name)] = rec
    name, win = windows(n, False)[0]
    best = None
    for _ in range(a.repeats + 1):
        ctx.tfm(slots, slots, y, fs, window=win)
        ms = ctx.get_option("tfm_kernel_ms")
        best = ms if best is None else min(best, ms)
    out["tfm_" + name] = {"tfm_kernel_ms": round(best, 2), "tfm_upload_ms": round(ctx.get_option("tfm_upload_ms"), 2)}
    ctx.close()
    out["notes"] = ("kernel ms: HIP events in the library; upload / download ms: the pageable hipMemcpy of the float32 traces "
                    "down and of the complex64 result up, host clock in the library; call ms: wall clock of "
                    "Context.trace_spectral; each the best of %d; numpy route: wall clock on this host's CPUs in the same "
                    "session" % a.repeats)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
