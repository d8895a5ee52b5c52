"""TFM imaging from resident fields (alifmm_tfm) on the 4096^2 weld-like workload (GPU box):
64 elements on the top row, their fields computed by travel(copy_out=False) and left on the device,
synthetic complex data with nt = 4096, windows 1024^2 and 4096^2 at step 1.  Per window: upload ms
(data, weights and slot table to the device), kernel ms (best of the repeats) and terms/s
(pairs x pixels / kernel time; fs is chosen so that every delay is in range).  Two variants of the
4096^2 run separate the kernel's costs: "one_sample" (fs so low that every term reads samples 0
and 1: the same arithmetic without divergent gather addresses) and "out_of_range" (t0 past every
delay: the term is branch-free, so this too reads samples 0 and 1 and does all the arithmetic; it
showed the cost of the skipped terms while the term still branched).  "chunk_sweep": kernel ms of
the 4096^2 window per value of option tfm_chunk.  "copy_fields_ms": the same 64 fields returned to pageable host memory
(alifmm_copy_fields), the only way to the same image without alifmm_tfm.
python tools/tfm_bench.py [--n 4096] [--elements 64] [--nt 4096] [--repeats 3]  -> one JSON line"""
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
import workloads as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--elements", type=int, default=64)
    ap.add_argument("--nt", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-copy", action="store_true", help="skip the copy_fields leg")
    a = ap.parse_args()
    n, ne, nt = a.n, a.elements, a.nt
    ctx = _alifmm.Context(0)
    vt = W.default_table()
    ctx.set_model(*W.weldlike_model(n), vt, vt, W.weldlike_dnx())
    sx, sz = W.c4_sources(ne, n)
    t = time.perf_counter()
    ctx.travel(sx, sz, copy_out=False)
    travel_s = time.perf_counter() - t
    # the largest delay: the far bottom corner of the first / last element's field
    tmax = max(ctx.get_field(0, 1).max(), ctx.get_field(ne - 1, 1).max())
    fs = (nt - 2) / (2.0 * tmax)
    rng = np.random.default_rng(5)
    fmc = rng.standard_normal((ne, ne, nt, 2), dtype=np.float32).view(np.complex64)[..., 0]
    slots = list(range(ne))
    out = {"n": n, "elements": ne, "nt": nt, "fs_hz": fs, "travel_s": round(travel_s, 3),
           "tfm_chunk": int(ctx.get_option("tfm_chunk")), "data_MB": round(fmc.nbytes / 1e6, 1)}

    def run(window, fs_=fs, t0=0.0):
        best = None
        for _ in range(a.repeats):
            t = time.perf_counter()
            img = ctx.tfm(slots, slots, fmc, fs_, t0=t0, window=window)
            wall = time.perf_counter() - t
            rec = {"upload_ms": round(ctx.get_option("tfm_upload_ms"), 2),
                   "kernel_ms": round(ctx.get_option("tfm_kernel_ms"), 3), "wall_ms": round(1e3 * wall, 1)}
            if best is None or rec["kernel_ms"] < best["kernel_ms"]:
                best = rec
        terms = ne * ne * window[2] * window[3]
        best["terms"] = terms
        best["terms_per_s"] = float("%.4g" % (terms / (1e-3 * best["kernel_ms"])))
        best["image_abs_mean"] = float(np.abs(img).mean())
        return best

    w_small = min(1024, n)
    o = (n - w_small) // 2
    run((o, o, min(256, n), min(256, n)))  # warm-up: code object, buffers
    out["window_%d" % w_small] = run((o, o, w_small, w_small))
    full = (0, 0, n, n)
    out["window_%d" % n] = run(full)
    out["one_sample"] = run(full, fs_=0.25 / tmax)
    out["out_of_range"] = run(full, t0=4.0 * tmax)
    sweep = {}
    for c in (4, 8, 16, 32):
        ctx.set_option("tfm_chunk", c)
        sweep[str(c)] = run(full)["kernel_ms"]
    ctx.set_option("tfm_chunk", out["tfm_chunk"])
    out["chunk_sweep_kernel_ms"] = sweep
    if not a.no_copy:
        fz, fx = ctx.field_shape(1)
        D = np.empty((ne, fz, fx))
        D.fill(0.0)  # touch the pages first: the copy is timed, not the page faults
        best = None
        for _ in range(2):
            t = time.perf_counter()
            ctx.copy_fields(0, ne, 1, out=D)
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        out["copy_fields_ms"] = round(1e3 * best, 1)
        out["copy_fields_GB"] = round(D.nbytes / 1e9, 2)
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
