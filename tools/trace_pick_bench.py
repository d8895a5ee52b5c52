"""The time-of-flight picker (alifmm_trace_pick) against the only route there was before it (GPU
box): 64 x 64 real float32 RF traces of 4096 samples, one echo of a 64-tap pulse per trace in noise,
made analytic, band-passed (2 .. 8 MHz at fs 40 MHz) and matched-filtered in one pass, picked in
256-sample gates around the echoes.
  - Context.trace_pick with the filter resident: the whole call's wall ms and its four parts
    (upload, filter kernel, pick kernel, download; alifmm_get_option), best of the repeats;
  - in the same session the old route: Context.trace_spectral with the same response (the analytic
    cube comes back to the host), then numpy on the host over the same gates: |y|, argmax, the
    parabola through the three amplitudes; its wall ms and the filter's parts;
  - both at the transform length pick_times() chooses for this pulse (8192: nt + ntap - 1 does not
    wrap) and at 4096;
  - the two routes' picks compared (they differ only where numpy's float32 |y| ties or rounds
    otherwise than the float64 rule).
python tools/trace_pick_bench.py [--elements 64] [--nt 4096] [--repeats 5] [--out FILE]
-> one JSON line, also written to FILE (default profiles/trace_pick_bench.json)"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ali-fmm-and-ray-tracing_amd"))
import _alifmm  # noqa: E402


def numpy_pick(y, lo, width):
    """argmax of |y| over [lo, lo + width) per trace and the parabola's vertex, vectorised."""
    cols = lo[:, None] + np.arange(width)[None, :]
    a = np.abs(np.take_along_axis(y, cols, axis=1)).astype(np.float64)
    k = np.argmax(a, axis=1)
    m = lo + k
    r = np.arange(len(m))
    nt = y.shape[1]
    am, a0, ap = np.abs(y[r, np.maximum(m - 1, 0)]).astype(np.float64), a[r, k], np.abs(y[r, np.minimum(m + 1, nt - 1)]).astype(np.float64)
    den = (am - 2 * a0) + ap
    ok = (m > 0) & (m < nt - 1) & (am <= a0) & (ap <= a0) & (den < 0)
    return m + np.where(ok, 0.5 * (am - ap) / np.where(ok, den, 1.0), 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=64)
    ap.add_argument("--nt", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trace_pick_bench.json"))
    a = ap.parse_args()
    ne, nt, fs, ntap, width = a.elements, a.nt, 40e6, 64, 256
    ntrace = ne * ne
    rng = np.random.default_rng(5)
    k = np.arange(ntap) - ntap // 2
    pulse = np.exp(-0.5 * (k / 8.0) ** 2) * np.cos(2 * np.pi * (5e6 / fs) * k)  # 5 MHz, origin ntap // 2
    delay = rng.integers(300, nt - 300, ntrace)
    rf = 0.05 * rng.standard_normal((ntrace, nt))
    for t in range(ntrace):
        rf[t, delay[t] - ntap // 2:delay[t] - ntap // 2 + ntap] += pulse
    rf = rf.astype(np.float32)
    lo = (delay - width // 2 + rng.integers(-40, 40, ntrace)).astype(np.int32)
    hi = lo + width
    ctx = _alifmm.Context(0)
    ctx.trace_pick(rf[:1], lo[:1], hi[:1], analytic=True)  # warm-up: the code objects
    out = {"elements": ne, "nt": nt, "fs_hz": fs, "ntap": ntap, "gate": width, "rf_MB_f32": round(rf.nbytes / 1e6, 1),
           "analytic_MB_c64": round(2 * rf.nbytes / 1e6, 1), "n_cu": int(ctx.get_option("n_cu")),
           "trace_pick_grid": int(ctx.get_option("trace_pick_grid")), "host_cpus": len(os.sched_getaffinity(0))}
    for nfft in (2 * nt, nt):
        h = _alifmm.matched_response(nfft, pulse, ntap // 2) * _alifmm.bandpass_response(nfft, fs, 2e6, 8e6)
        new, old = {}, {}
        for _ in range(a.repeats + 1):  # (the first call grows the buffers)
            t = time.perf_counter()
            pos, amp, idx, amp2, idx2, flags = ctx.trace_pick(rf, lo, hi, guard=ntap, response=h, analytic=True, nfft=nfft)
            got = {"call_ms": 1e3 * (time.perf_counter() - t)}
            got.update({p + "_ms": ctx.get_option("trace_pick_%s_ms" % p) for p in ("upload", "filter", "kernel", "download")})
            new = {k_: min(v, new.get(k_, v)) for k_, v in got.items()}
            t = time.perf_counter()
            y = ctx.trace_spectral(rf, response=h, analytic=True, nfft=nfft)
            t1 = time.perf_counter()
            ref = numpy_pick(y, lo.astype(np.int64), width)
            t2 = time.perf_counter()
            got = {"call_ms": 1e3 * (t2 - t), "trace_spectral_ms": 1e3 * (t1 - t), "numpy_pick_ms": 1e3 * (t2 - t1)}
            got.update({p + "_ms": ctx.get_option("trace_fft_%s_ms" % p) for p in ("upload", "kernel", "download")})
            old = {k_: min(v, old.get(k_, v)) for k_, v in got.items()}
        rec = {"trace_pick": {k_: round(v, 3) for k_, v in new.items()},
               "trace_spectral_then_numpy": {k_: round(v, 3) for k_, v in old.items()},
               "old_over_new_call": round(old["call_ms"] / new["call_ms"], 2),
               "picks_within_1e-3_sample_of_numpy": float(np.mean(np.abs(pos - ref) <= 1e-3)),
               "max_abs_pick_minus_delay": float(np.abs(pos - delay).max()), "flags_set": int(np.count_nonzero(flags))}
        out["nfft_%d" % nfft] = rec
    ctx.close()
    out["notes"] = ("kernel ms: HIP events in the library; upload / download ms: pageable hipMemcpy, host clock in the library; "
                    "call ms: wall clock of the Python call(s); each the best of %d; the numpy pick runs on this host's CPUs in "
                    "the same session" % a.repeats)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
