"""Coherence-weighted TFM (alifmm_tfm_coh) next to the plain delay-and-sum (alifmm_tfm) on the 4096^2
weld-like workload of tools/tfm_bench.py (GPU box): 64 elements on the top row, their fields computed
by travel(copy_out=False) and left on the device, 64 x 64 synthetic complex A-scans with nt = 4096
(fs chosen so that every delay is in range), windows 1024^2 and 4096^2 at step 1.  Per window, in one
run on the same data: tfm_kernel_ms of alifmm_tfm and tfm_coh_kernel_ms of kinds 1 (CF), 2 (SCF) and
3 (PCF), each the best of the repeats, and the ratios over alifmm_tfm.  The legs alternate within a
repeat, so a drift of the clocks falls on all four alike.  The images are compared on the way
(alifmm_tfm_coh's must have alifmm_tfm's bits).
python tools/tfm_coh_bench.py [--n 4096] [--elements 64] [--nt 4096] [--repeats 3]  -> one JSON line,
also written to profiles/tfm_coh_bench.json with --write"""
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

KINDS = ("cf", "scf", "pcf")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--elements", type=int, default=64)
    ap.add_argument("--nt", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--write", metavar="PATH", nargs="?", const=os.path.join(REPO, "profiles", "tfm_coh_bench.json"),
                    help="also write the JSON line to PATH (default profiles/tfm_coh_bench.json)")
    a = ap.parse_args()
    n, ne, nt = a.n, a.elements, a.nt
    ctx = _alifmm.Context(0)
    vt = W.default_table()
    ctx.set_model(*W.weldlike_model(n), vt, vt, W.weldlike_dnx())
    sx, sz = W.c4_sources(ne, n)
    t = time.perf_counter()
    ctx.travel(sx, sz, copy_out=False)
    travel_s = time.perf_counter() - t
    tmax = max(ctx.get_field(0, 1).max(), ctx.get_field(ne - 1, 1).max())
    fs = (nt - 2) / (2.0 * tmax)
    rng = np.random.default_rng(5)
    fmc = rng.standard_normal((ne, ne, nt, 2), dtype=np.float32).view(np.complex64)[..., 0]
    slots = list(range(ne))
    out = {"n": n, "elements": ne, "nt": nt, "fs_hz": fs, "travel_s": round(travel_s, 3),
           "tfm_chunk": int(ctx.get_option("tfm_chunk")), "data_MB": round(fmc.nbytes / 1e6, 1)}

    def run(window):
        best = {}
        for _ in range(a.repeats):
            plain = ctx.tfm(slots, slots, fmc, fs, window=window)
            ms = {"tfm": ctx.get_option("tfm_kernel_ms")}
            for kind in KINDS:
                img, fac = ctx.tfm_coh(slots, slots, fmc, fs, kind=kind, window=window)
                ms[kind] = ctx.get_option("tfm_coh_kernel_ms")
                if not np.array_equal(img, plain):
                    raise SystemExit("tfm_coh (%s): the image differs from tfm's" % kind)
                best["factor_mean_" + kind] = float(fac.mean())
            for k, v in ms.items():
                best[k] = v if k not in best else min(best[k], v)
        rec = {"tfm_kernel_ms": round(best["tfm"], 3)}
        for kind in KINDS:
            rec["tfm_coh_kernel_ms_" + kind] = round(best[kind], 3)
            rec["ratio_" + kind] = round(best[kind] / best["tfm"], 3)
            rec["factor_mean_" + kind] = best["factor_mean_" + kind]
        rec["terms"] = ne * ne * window[2] * window[3]
        return rec

    w_small = min(1024, n)
    o = (n - w_small) // 2
    run((o, o, min(256, n), min(256, n)))  # warm-up: code objects, buffers
    out["window_%d" % w_small] = run((o, o, w_small, w_small))
    out["window_%d" % n] = run((0, 0, n, n))
    line = json.dumps(out)
    print(line, flush=True)
    if a.write:
        with open(a.write, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
