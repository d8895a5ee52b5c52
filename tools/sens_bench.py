"""Travel-time sensitivities along rays kept on the device (alifmm_ray_sens) on the 4096^2 weld-like
workload (GPU box): receivers on the bottom surface, 256 top-surface sources per receiver (the C5
trans_pairs pattern, tools/ray_bench.py), rays traced through the resident receiver fields at
subgrid 1 with their points kept on the device.  Reports, best of the repeats: sens_kernel_ms (count
and fill kernels) for the maps alone and for maps plus rows, the entries and entries/s, the shortest
wall time of each call (maps plus rows: the count call, the fill call and the rows' copy to the host), beside
ray_kernel_ms of tracing the same rays and take_rays_ms, the copy of their points to the host: the
first leg of the only other route to the same numbers (the second, a Python loop over
time_between_points(), is not measured).
python tools/sens_bench.py [--receivers 16] [--repeats 3] [--out FILE]  -> one JSON line; FILE (e.g.
profiles/sens_bench.json) collects the runs, one per request size, under the key receivers_N"""
import argparse
import ctypes
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
    ap.add_argument("--receivers", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, nrec = a.n, a.receivers
    ctx = _alifmm.Context(0)
    L = _alifmm.lib()
    vt = W.default_table()
    dnx = W.weldlike_dnx()
    ctx.set_model(*W.weldlike_model(n), vt, vt, dnx)
    step = n // 256
    rx = step // 2 + step * np.arange(256)[:: 256 // nrec][:nrec]
    t = time.perf_counter()
    ctx.travel(dnx * rx.astype(float), np.full(len(rx), dnx * (n - 1)), first_slot=0, copy_out=False)
    travel_s = time.perf_counter() - t
    src = np.stack([step // 2 + float(step) * np.arange(256), np.zeros(256)], 1)
    slots = np.repeat(np.arange(nrec, dtype=np.int32), 256)
    s_xy = np.ascontiguousarray(np.tile(src, (nrec, 1)))
    r_xy = np.ascontiguousarray(np.repeat(np.stack([rx.astype(float), np.full(nrec, float(n - 1))], 1), 256, axis=0))
    nr = len(slots)
    times, lens, flags = np.zeros(nr), np.zeros(nr, dtype=np.int32), np.zeros(nr, dtype=np.int32)

    def trace():
        rc = L.alifmm_find_rays(ctx._h, nr, slots.ctypes.data, s_xy.ctypes.data, r_xy.ctypes.data, times.ctypes.data,
                                lens.ctypes.data, flags.ctypes.data, None, _alifmm.KEEP_RAYS)
        assert rc == 0, L.alifmm_last_error(ctx._h)

    trace()  # warm-up: code objects, buffers
    trace()
    out = {"n": n, "receivers": nrec, "rays": nr, "points": int(lens.sum(dtype=np.int64)), "travel_s": round(travel_s, 3),
           "ray_kernel_ms": round(ctx.get_option("ray_kernel_ms"), 3), "find_rays_ms": round(ctx.get_option("find_rays_ms"), 3),
           "rays_cut_short": int(np.count_nonzero(flags & 6))}

    def run(rows):
        best, walls = None, []
        for _ in range(a.repeats + 1):  # the first repeat allocates the buffers
            t = time.perf_counter()
            maps, csr, status = ctx.ray_sens(lens, None, subgrid=1, flags=flags, maps=True, rows=rows)
            wall = time.perf_counter() - t
            rec = {"sens_kernel_ms": round(ctx.get_option("sens_kernel_ms"), 3), "wall_ms": round(1e3 * wall, 2),
                   "sens_upload_ms": round(ctx.get_option("sens_upload_ms"), 3)}
            walls.append(rec["wall_ms"])
            if best is None or rec["sens_kernel_ms"] < best["sens_kernel_ms"]:
                best = rec
        best["wall_ms"] = min(walls)  # (the first calls also fault in the fresh result arrays)
        entries = int(ctx.get_option("sens_entries"))
        best["entries_per_s"] = float("%.4g" % (entries / (1e-3 * best["sens_kernel_ms"])))
        return best, entries, maps, csr, status

    m_only, entries, maps, _, status = run(False)
    m_rows, _, maps2, csr, _ = run(True)
    out.update({"entries": entries, "invalid_rays": int(status.sum()), "maps_only": m_only, "maps_and_rows": m_rows,
                "rows_MB": round(sum(v.nbytes for v in csr[1:]) / 1e6, 1),
                # the sum of the time map is the sum of the rays' times (those not cut short)
                "time_map_sum_rel_err": float(abs(maps[1].sum() - times.sum()) / times.sum()),
                "maps_max_rel_diff_between_calls": float(np.max(np.abs(maps - maps2)) / np.max(np.abs(maps)))})
    pts = np.empty((out["points"], 2))
    got = ctypes.c_int64(0)
    rc = L.alifmm_take_rays(ctx._h, pts.ctypes.data, len(pts), ctypes.byref(got))
    assert rc == 0 and got.value == len(pts)
    out["take_rays_ms"] = round(ctx.get_option("take_rays_ms"), 3)
    out["points_MB"] = round(pts.nbytes / 1e6, 1)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        allr = {}
        if os.path.exists(a.out):  # one file for several request sizes
            with open(a.out) as f:
                allr = json.load(f)
        allr["receivers_%d" % nrec] = out
        with open(a.out, "w") as f:
            json.dump(allr, f, indent=1, sort_keys=True)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
