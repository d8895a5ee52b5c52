"""Reflected fields from resident incident fields (alifmm_travel_seeded) on the 4096^2 weld-like
workload (GPU box): 64 elements on the top row, their direct fields computed by
travel(copy_out=False) and left on the device, reflector = the grid's last row (4096 seeds + 4096
close cells = 8192 hand-over entries per field), the 64 reflected fields seeded from them in one
call.  Recorded: the seeded call's seed_ms, band_ms and total (best total of the repeats), beside
them the same run's 64 direct fields (alifmm_last_timing: the only comparable figure), the band
steps of a direct and of a reflected field, and the half-skip alifmm_tfm (reflected transmit fields,
direct receive fields) on the full grid.  No ratio is asserted.
python tools/seeded_bench.py [--n 4096] [--elements 64] [--nt 4096] [--repeats 3]  -> one JSON line"""
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
    ap.add_argument("--no-tfm", action="store_true", help="skip the half-skip TFM leg")
    a = ap.parse_args()
    n, ne, nt = a.n, a.elements, a.nt
    ctx = _alifmm.Context(0)
    vt = W.default_table()
    ctx.set_model(*W.weldlike_model(n), vt, vt, W.weldlike_dnx())
    sx, sz = W.c4_sources(ne, n)
    wall_iz, wall_ix = np.full(n, n - 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    out = {"n": n, "elements": ne, "reflector": "last row"}

    def timing(wall):
        i, b, t = ctx.last_timing()
        return {"init_ms": round(i, 3), "band_ms": round(b, 2), "total_ms": round(t, 2), "wall_ms": round(1e3 * wall, 1),
                "members": int(ctx.get_option("last_k"))}

    direct = seeded = None
    for _ in range(a.repeats):
        ctx.set_option("init_reuse", 0)  # every repeat walks its source inits: the direct figure is a cold one
        t = time.perf_counter()
        ctx.travel(sx, sz, copy_out=False)
        rec = timing(time.perf_counter() - t)
        if direct is None or rec["total_ms"] < direct["total_ms"]:
            direct = rec
        t = time.perf_counter()
        ctx.travel_seeded(wall_iz, wall_ix, from_slots=list(range(ne)), first_slot=ne, copy_out=False)
        rec = timing(time.perf_counter() - t)
        rec["seed_ms"] = round(ctx.get_option("seed_ms"), 3)
        if seeded is None or rec["total_ms"] < seeded["total_ms"]:
            seeded = rec
    out["direct"] = direct
    out["seeded"] = seeded
    out["seed_nodes"] = int(ctx.get_option("seed_nodes"))
    out["seed_close"] = int(ctx.get_option("seed_close"))
    out["band_ms_ratio_seeded_to_direct"] = round(seeded["band_ms"] / direct["band_ms"], 3)
    out["steps_direct"] = int(ctx.source_stats(ne // 2)[0][3])
    out["steps_seeded"] = int(ctx.source_stats(ne + ne // 2)[0][3])
    out["sweeps_direct"] = int(ctx.source_stats(ne // 2)[1])
    out["sweeps_seeded"] = int(ctx.source_stats(ne + ne // 2)[1])
    if not a.no_tfm:
        tmax = ctx.get_field(ne, 1).max() + ctx.get_field(0, 1).max()
        fs = (nt - 2) / tmax
        rng = np.random.default_rng(5)
        fmc = rng.standard_normal((ne, ne, nt, 2), dtype=np.float32).view(np.complex64)[..., 0]
        tx, rx = list(range(ne, 2 * ne)), list(range(ne))
        ctx.tfm(tx, rx, fmc, fs, window=(0, 0, min(256, n), min(256, n)))  # warm-up
        best = None
        for _ in range(a.repeats):
            t = time.perf_counter()
            img = ctx.tfm(tx, rx, fmc, fs)
            wall = time.perf_counter() - t
            rec = {"upload_ms": round(ctx.get_option("tfm_upload_ms"), 2),
                   "kernel_ms": round(ctx.get_option("tfm_kernel_ms"), 3), "wall_ms": round(1e3 * wall, 1)}
            if best is None or rec["kernel_ms"] < best["kernel_ms"]:
                best = rec
        best["image_abs_mean"] = float(np.abs(img).mean())
        out["tfm_half_skip"] = best
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
