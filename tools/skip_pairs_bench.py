"""Back-wall echo paths between element pairs (alifmm_skip_pick / alifmm_skip_rays) on the 4096^2
weld-like workload (GPU box): 64 elements on the top row, their direct fields computed by
travel(copy_out=False) and left on the device, every pair i <= j (2080), the back wall = the grid's
last row (4096 nodes).  Recorded: skip_pick_ms of the pick alone and of the rays call, skip_join_ms,
the ray kernel's time and the whole call (best of the repeats), and beside them, from the same run,
the two routes to an echo time that existed before: returning the 64 fields to the host
(alifmm_copy_fields, after which the host would reduce them) and the 64 reflected fields of
skip_fields (alifmm_travel_seeded from the resident direct fields).  No ratio is asserted.
python tools/skip_pairs_bench.py [--n 4096] [--elements 64] [--repeats 3] [--out profiles/skip_pairs_bench.json]"""
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "skip_pairs_bench.json"))
    ap.add_argument("--no-copy", action="store_true", help="skip the copy of the fields to the host")
    a = ap.parse_args()
    n, ne = a.n, a.elements
    ctx = _alifmm.Context(0)
    vt = W.default_table()
    dnx = W.weldlike_dnx()
    ctx.set_model(*W.weldlike_model(n), vt, vt, dnx)
    sx, sz = W.c4_sources(ne, n)
    ex = np.round(sx / dnx)
    wall_iz, wall_ix = np.full(n, n - 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    ii, jj = np.nonzero(np.triu(np.ones((ne, ne))))
    xy = np.stack([ex, np.zeros(ne)], axis=1)
    out = {"n": n, "elements": ne, "pairs": int(len(ii)), "reflector_nodes": n, "reflector": "last row"}

    t = time.perf_counter()
    ctx.travel(sx, sz, copy_out=False)
    out["direct_fields"] = {"total_ms": round(ctx.last_timing()[2], 2), "wall_ms": round(1e3 * (time.perf_counter() - t), 1)}

    pick = rays = None
    for _ in range(a.repeats):
        t = time.perf_counter()
        pt, hit = ctx.skip_pick(ii, jj, wall_iz, wall_ix)
        rec = {"skip_pick_ms": round(ctx.get_option("skip_pick_ms"), 4), "wall_ms": round(1e3 * (time.perf_counter() - t), 2)}
        if pick is None or rec["skip_pick_ms"] < pick["skip_pick_ms"]:
            pick = rec
        t = time.perf_counter()
        r = ctx.skip_rays(ii, jj, xy[ii], xy[jj], wall_iz, wall_ix, with_points="keep", check=False)
        rec = {k: round(ctx.get_option(k), 4) for k in ("skip_pick_ms", "skip_join_ms", "ray_kernel_ms", "find_rays_ms")}
        rec["wall_ms"] = round(1e3 * (time.perf_counter() - t), 2)
        rec["ray_lanes"] = int(ctx.get_option("ray_lanes"))
        if rays is None or rec["find_rays_ms"] < rays["find_rays_ms"]:
            rays = rec
    out["pick"] = pick
    out["rays"] = rays
    out["hits"] = int(np.count_nonzero(hit >= 0))
    out["points"] = int(r[3].sum(dtype=np.int64))
    out["flags_or"] = int(np.bitwise_or.reduce(r[4]))
    # pulse-echo: the mirror point of element i is below it
    pe = ii == jj
    out["pulse_echo_hit_offset_max_nodes"] = float(np.max(np.abs(wall_ix[hit[pe]] - ex[ii[pe]])))
    out["pick_vs_ray_time_rel_max"] = float(np.max(np.abs(r[2] - pt) / pt))

    # the routes that existed before
    if not a.no_copy:
        best = None
        dst = np.empty((ne,) + ctx.field_shape(1))
        for _ in range(a.repeats):
            t = time.perf_counter()
            _, gbps = ctx.copy_fields(0, ne, 1, out=dst)
            rec = {"wall_ms": round(1e3 * (time.perf_counter() - t), 1), "gbps": round(gbps, 2)}
            if best is None or rec["wall_ms"] < best["wall_ms"]:
                best = rec
        out["copy_fields_to_host"] = best
        del dst
    best = None
    for _ in range(a.repeats):
        t = time.perf_counter()
        ctx.travel_seeded(wall_iz, wall_ix, from_slots=list(range(ne)), first_slot=ne, copy_out=False)
        i, b, tot = ctx.last_timing()
        rec = {"seed_ms": round(ctx.get_option("seed_ms"), 3), "band_ms": round(b, 2), "total_ms": round(tot, 2),
               "wall_ms": round(1e3 * (time.perf_counter() - t), 1)}
        if best is None or rec["total_ms"] < best["total_ms"]:
            best = rec
    out["skip_fields_reflected"] = best
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
