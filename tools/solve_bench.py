"""The resident sensitivity operator (alifmm_sens_op_build / _apply / _solve) on the 4096^2 weld-like
workload of tools/sens_bench.py (GPU box): receivers on the bottom surface, 256 top-surface sources
per receiver, rays traced through the resident receiver fields at subgrid 1 with their points kept
on the device; the operator is the Jacobian in the velocity scale (quantity 1, col_scale =
-1 / vel_map).  Reports, best of the repeats: solve_build_ms (the whole build: count and fill passes,
the transposed copy, the column lists), the device time of one product in each direction and of one
CGLS iteration (a solve of --iters iterations with tol = 0, divided by the iterations: its start, one
Aᵀ product and two norms, is inside), each beside its floor = the bytes the step must move at
8 TB/s, and the fraction of the floor reached; beside them the route this replaces, the rows copied
to the host before any host solve starts (profiles/sens_bench.json maps_and_rows.wall_ms).
Bytes: a product streams 12 B per entry (int32 + float64) and the vectors it gathers and writes once;
an iteration is both products and the passes of the fused vector kernels.
python tools/solve_bench.py [--receivers 16] [--repeats 3] [--iters 20] [--out FILE]  -> one JSON line;
FILE (e.g. profiles/solve_bench.json) collects the runs under the key receivers_N"""
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

PEAK = 8e12  # HBM3E, bytes / s


def floors(entries, ncell, nrays):
    """Bytes each step must move: (A x, Aᵀ y, one CGLS iteration).  Vectors of cells: A x gathers cs
    and x; Aᵀ y zeroes and writes the result and reads cs; the iteration adds the passes of the
    fused kernels (|q|²: p and the mask; update: x, p, x; s: t, x, mask, s; p: s, p, p)."""
    ax = 12 * entries + 8 * (2 * ncell + nrays)
    aty = 12 * entries + 8 * (3 * ncell + nrays)
    it = ax + aty + 8 * (12 * ncell + 5 * nrays)
    return ax, aty, it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--receivers", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, nrec = a.n, a.receivers
    ctx = _alifmm.Context(0)
    L = _alifmm.lib()
    vt = W.default_table()
    dnx = W.weldlike_dnx()
    model = W.weldlike_model(n)
    ctx.set_model(*model, vt, vt, dnx)
    step = n // 256
    rx = step // 2 + step * np.arange(256)[:: 256 // nrec][:nrec]
    ctx.travel(dnx * rx.astype(float), np.full(len(rx), dnx * (n - 1)), first_slot=0, copy_out=False)
    src = np.stack([step // 2 + float(step) * np.arange(256), np.zeros(256)], 1)
    slots = np.repeat(np.arange(nrec, dtype=np.int32), 256)
    s_xy = np.ascontiguousarray(np.tile(src, (nrec, 1)))
    r_xy = np.ascontiguousarray(np.repeat(np.stack([rx.astype(float), np.full(nrec, float(n - 1))], 1), 256, axis=0))
    nr = len(slots)
    times, lens, flags = np.zeros(nr), np.zeros(nr, dtype=np.int32), np.zeros(nr, dtype=np.int32)
    rc = L.alifmm_find_rays(ctx._h, nr, slots.ctypes.data, s_xy.ctypes.data, r_xy.ctypes.data, times.ctypes.data,
                            lens.ctypes.data, flags.ctypes.data, None, _alifmm.KEEP_RAYS)
    assert rc == 0, L.alifmm_last_error(ctx._h)
    ncell = n * n
    cs = -1.0 / np.asarray(model[2], dtype=np.float64)
    rng = np.random.default_rng(1)
    x, y = rng.normal(size=ncell), 1e-8 * rng.normal(size=nr)

    build, walls = [], []
    for _ in range(a.repeats):
        t = time.perf_counter()
        entries, status = ctx.sens_op_build(lens, None, subgrid=1, flags=flags, quantity=1, col_scale=cs)
        walls.append(1e3 * (time.perf_counter() - t))
        build.append(ctx.get_option("solve_build_ms"))
    f_ax, f_aty, f_it = floors(entries, ncell, nr)

    def product(v, transpose):
        best, first = None, None
        for _ in range(a.repeats + 1):  # the first repeat allocates the vectors
            out = ctx.sens_op_apply(v, transpose=transpose)
            ms = ctx.get_option("solve_kernel_ms")
            best = ms if best is None else min(best, ms)
            same = True if first is None else bool(np.array_equal(first.view(np.int64), out.view(np.int64)))
            first = out if first is None else first
            assert same, "a product changed its bits between two calls"
        return best, first

    ax_ms, ax = product(x, False)
    aty_ms, aty = product(y, True)
    unit = float(np.linalg.norm(aty)) / max(float(np.linalg.norm(y)), 1e-300) / np.sqrt(ncell)
    it_ms, info = None, None
    for _ in range(a.repeats):
        _, info = ctx.sens_op_solve(y, damp=unit, smooth=unit, max_iter=a.iters, tol=0.0)
        ms = ctx.get_option("solve_kernel_ms") / max(info["iterations"], 1)
        it_ms = ms if it_ms is None else min(it_ms, ms)

    def rec(ms, floor_bytes):
        fl = 1e3 * floor_bytes / PEAK
        return {"ms": round(ms, 3), "floor_ms": round(fl, 3), "MB": round(floor_bytes / 1e6, 1),
                "fraction_of_floor": round(fl / ms, 3)}

    out = {"n": n, "receivers": nrec, "rays": nr, "entries": int(entries), "invalid_rays": int(status.sum()),
           "rays_cut_short": int(np.count_nonzero(flags & 6)), "operator_MB": round(24 * entries / 1e6, 1),
           "build_ms": round(min(build), 2), "build_call_wall_ms": round(min(walls), 2),
           "apply": rec(ax_ms, f_ax), "apply_transpose": rec(aty_ms, f_aty), "cgls_iteration": rec(it_ms, f_it),
           "cgls": {"iterations": info["iterations"], "reason": info["reason"], "grad_over_grad0": info["grad"] / info["grad0"],
                    "res_over_rhs": info["res_norm"] / info["rhs_norm"]},
           "peak_bytes_per_s": PEAK, "products_bit_identical_between_calls": True}
    sens = os.path.join(REPO, "profiles", "sens_bench.json")
    if os.path.exists(sens):  # the route this replaces: measured by tools/sens_bench.py, not here
        with open(sens) as f:
            prev = json.load(f).get("receivers_%d" % nrec)
        if prev:
            out["rows_to_host_wall_ms_from_sens_bench"] = prev["maps_and_rows"]["wall_ms"]
            out["rows_MB_from_sens_bench"] = prev["rows_MB"]
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
