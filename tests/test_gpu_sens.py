"""Travel-time sensitivities along rays on the device (csrc/ray_sens.hip, host_sens.cpp alifmm_ray_sens,
Context.ray_sens, ALI_FMM.ray_sensitivity) against the Python restatement of the contract
(tests/sens_ref.py, pinned to the oracle by tests/test_sens_ref.py) with the correctly rounded build
of the oracle.  Fields are uploaded (alifmm_put_field) where rays are traced.  Run: pytest -m gpu.

Bars against the restatement: entry counts, col and len equal; time <= 1e-12 relative (the project's
bar for times); |dth - ref| <= 2^-40 time_ref (each of the two slownesses of the centred difference
may move by one ulp, 2^-52 s; the difference is scaled by 512; times 4).  Maps: per cell
|map - np.add.at(reference rows)| <= N_c 2^-52 sum|terms|, N_c the cell's entry count (the float64
atomic adds arrive in no fixed order).  The worst figures go to the session's parity envelope under
"sens/..." before anything is asserted.

Measured on the MI355X when the file was written: every entry of every group bit-equal to the
restatement (time and dth: worst 0, 100 % exact), rows through the kept points bit-identical to rows
through ray_xy, maps at most 0.35 of their bound (up to 36 entries per cell), the drop-in's per-ray
time sums within 6.4e-16 of the times matrix.
"""
import ctypes

import numpy as np
import pytest

import ray_cases as RC
import sens_ref as SR

pytestmark = pytest.mark.gpu

EXACT = 1e-12
DTH = 2.0 ** -40
MAP = 2.0 ** -52


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    yield c
    c.close()


_ref_models = {}


def _ref_model(m):
    key = (m.name, m.nz, m.nx)
    if key not in _ref_models:
        _ref_models[key] = SR.Model(m)
    return _ref_models[key]


def _vs_ref(envelope, name, got, status, want):
    """A request's CSR (row_ptr, col, len, time, dth) and status against the restatement's; the
    figures are recorded before anything is asserted."""
    counts = np.array_equal(got[0], want[0])
    stat = np.array_equal(status, want[5])
    rec = {"rays": len(want[5]), "entries": int(want[0][-1]), "counts_equal": counts, "status_equal": stat}
    if counts:
        t_ref = want[3]
        rel = np.abs(got[3] - t_ref) / np.where(t_ref != 0, np.abs(t_ref), 1.0)
        derr = np.abs(got[4] - want[4]) / np.where(t_ref != 0, np.abs(t_ref), 1.0)
        rec.update({"col_equal": bool(np.array_equal(got[1], want[1])), "len_equal": bool(np.array_equal(got[2], want[2])),
                    "time_rel_max": float(rel.max()) if rel.size else 0.0,
                    "time_exact_frac": float(np.mean(got[3] == t_ref)) if rel.size else 1.0,
                    "dth_err_over_time_max": float(derr.max()) if derr.size else 0.0,
                    "dth_exact_frac": float(np.mean(got[4] == want[4])) if derr.size else 1.0})
    envelope["sens/" + name] = rec
    assert counts and stat, (name, rec)
    assert rec["col_equal"] and rec["len_equal"], (name, rec)
    assert rec["time_rel_max"] <= EXACT, (name, rec)
    assert np.all(np.abs(got[4] - want[4]) <= DTH * np.abs(want[3])), (name, rec)
    return rec


def _same_rows(a, ka, b, kb):
    """Ray ka of CSR a and ray kb of CSR b hold the same bits."""
    sa, sb = slice(a[0][ka], a[0][ka + 1]), slice(b[0][kb], b[0][kb + 1])
    return all(np.array_equal(a[q][sa].view(np.int32 if q == 1 else np.int64), b[q][sb].view(np.int32 if q == 1 else np.int64))
               for q in (1, 2, 3, 4))


@pytest.mark.parametrize("mname,shape", RC.SEGMENT_RUNS, ids=["%s_%dx%d" % (m, s[0], s[1]) for m, s in RC.SEGMENT_RUNS])
def test_segment_matrix(ctx, envelope, mname, shape):
    """Every segment case as a two-point ray, subgrids 1 and 3, on the models of both instantiations
    (LDS tables: iso, stripes, mixed, m256; past them: m257, stif65, vt3): rows against the reference."""
    m = RC.model(mname, *shape)
    RC.set_model(ctx, m)
    for sg in RC.SEG_SUBGRIDS:
        ray_len, xy = SR.segments_request(RC.segments(shape, sg))
        _, csr, status = ctx.ray_sens(ray_len, xy, subgrid=sg, maps=False, rows=True)
        want = SR.rows(_ref_model(m), ray_len, xy, sg, RC.DNX)
        assert not want[5].any() and want[0][-1] > 2000
        _vs_ref(envelope, "segments/%s_%dx%d_sg%d" % (mname, shape[0], shape[1], sg), csr, status, want)
        assert ctx.get_option("sens_entries") == want[0][-1]


def _long_rays(nz, nx, sg, seed):
    """Synthetic rays of 1, 63, 64, 65, 127, 128, 129 and 200 segments: seeded points (multiples of
    1/64 of a fine node) each within 3 coarse nodes of the one before, inside the grid."""
    rng = np.random.default_rng(seed)
    rays = []
    for nseg in (1, 63, 64, 65, 127, 128, 129, 200):
        p = [np.array([rng.integers(0, 64 * sg * (nx - 1) + 1), rng.integers(0, 64 * sg * (nz - 1) + 1)]) / 64.0]
        while len(p) < nseg + 1:
            q = p[-1] + rng.integers(-3 * 64 * sg, 3 * 64 * sg + 1, 2) / 64.0
            q = np.minimum(np.maximum(q, 0.0), [sg * (nx - 1.0), sg * (nz - 1.0)])
            if q[1] == p[-1][1] and (q[1] / sg) % 1 == 0.5:  # (horizontal on a cell edge: may never end)
                continue
            if q[0] == p[-1][0] and (q[0] / sg) % 1 == 0.5:
                continue
            p.append(q)
        rays.append(np.array(p))
    return rays


WHOLE = RC.TRAVEL_BATCHES + [b for b in RC.DIST_BATCHES if b.sg == 9]


@pytest.mark.parametrize("b", WHOLE, ids=[b.name for b in WHOLE])
def test_whole_rays(ctx, envelope, b):
    """Rays traced on uploaded fields, once with their points copied out and once kept on the
    device: rows through ray_xy and through NULL are bit-identical, both meet the bars, the kept
    points are still there for take_rays; with them synthetic rays of 1 .. 200 segments (64, 65,
    128, 129: the wavefront's rounds) in a request whose last workgroup is partly filled."""
    import _alifmm

    L = _alifmm.lib()
    m = RC.model(b.model, b.nz, b.nx)
    RC.set_model(ctx, m)
    for k in range(len(b.fields)):
        ctx.put_field(k, b.sg, RC.field_array(b, k))
    slots = np.array([r[0] for r in b.rays], dtype=np.int32)
    src = np.array([r[1] for r in b.rays], dtype=np.float64)
    rec = np.array([r[2] for r in b.rays], dtype=np.float64)
    t, lens, flags, pts = ctx.find_rays(slots, src, rec, packed=True, check=False)
    n = len(lens)
    assert lens.min() == 2 and lens.max() > 20
    # through ray_xy, with the synthetic rays behind the traced ones
    extra = _long_rays(b.nz, b.nx, b.sg, 31)
    ray_len = np.concatenate([lens, [len(p) for p in extra]]).astype(np.int32)
    xy = np.concatenate([pts] + extra)
    fl = np.concatenate([flags, np.zeros(len(extra), dtype=np.int32)])
    assert len(ray_len) % 4 != 0
    _, host, status = ctx.ray_sens(ray_len, xy, subgrid=b.sg, flags=fl, maps=False, rows=True)
    want = SR.rows(_ref_model(m), ray_len, xy, b.sg, RC.DNX, fl)
    assert not want[5].any()
    _vs_ref(envelope, "whole/" + b.name, host, status, want)
    # a ray's time is the sum of its segments' sums; the entries sum piece by piece
    for k in range(n):
        if not (flags[k] & 6):
            s = float(np.sum(host[3][host[0][k]:host[0][k + 1]]))
            assert abs(s - t[k]) <= 1e-12 * max(t[k], 1e-300), (k, s, t[k])
    # kept on the device: the same rays traced again, their points never leaving the GPU
    t2, l2, f2 = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    rc = L.alifmm_find_rays(ctx._h, n, slots.ctypes.data, src.ctypes.data, rec.ctypes.data, t2.ctypes.data, l2.ctypes.data,
                            f2.ctypes.data, None, _alifmm.KEEP_RAYS)
    assert rc == 0 and np.array_equal(l2, lens) and np.array_equal(f2, flags)
    _, dev, dstatus = ctx.ray_sens(lens, None, subgrid=b.sg, flags=flags, maps=False, rows=True)
    assert np.array_equal(dev[0], host[0][:n + 1]) and not dstatus.any()
    first = next((k for k in range(n) if not _same_rows(dev, k, host, k)), None)
    envelope["sens/whole/" + b.name + "/kept_vs_host_first_difference"] = first
    assert first is None, first
    got = ctypes.c_int64(-1)
    back = np.empty_like(pts)
    assert L.alifmm_take_rays(ctx._h, back.ctypes.data, len(back), ctypes.byref(got)) == 0 and got.value == len(pts)
    assert np.array_equal(back, pts)


def _mix(ctx):
    """MIX_BATCH traced once: (lens, flags, per-ray point arrays)."""
    b = RC.MIX_BATCH
    RC.set_model(ctx, RC.model(b.model, b.nz, b.nx))
    for k in range(len(b.fields)):
        ctx.put_field(k, b.sg, RC.field_array(b, k))
    slots = np.array([r[0] for r in b.rays], dtype=np.int32)
    src = np.array([r[1] for r in b.rays], dtype=np.float64)
    rec = np.array([r[2] for r in b.rays], dtype=np.float64)
    t, lens, flags, pts = ctx.find_rays(slots, src, rec, packed=True, check=False)
    off = np.concatenate(([0], np.cumsum(lens, dtype=np.int64)))
    return lens, flags, [pts[off[k]:off[k + 1]] for k in range(len(lens))]


def _rows_of(ctx, rays, sg, flags=None):
    ray_len = np.array([len(p) for p in rays], dtype=np.int32)
    xy = np.concatenate(rays) if rays else np.zeros((0, 2))
    _, csr, status = ctx.ray_sens(ray_len, xy, subgrid=sg, flags=flags, maps=False, rows=True)
    return csr, status


def test_independence(ctx, envelope):
    """The MIX_BATCH list rotated and cut to 1, 3, 4, 5 rays (around a workgroup's 4 wavefronts):
    every ray's rows have the bits of the ray alone."""
    lens, flags, rays = _mix(ctx)
    n = len(rays)
    alone = [_rows_of(ctx, [rays[k]], 1, flags[k:k + 1])[0] for k in range(n)]
    assert sum(int(a[0][1]) for a in alone) > 500 and int(alone[RC.CAP_RAY][0][1]) == 0
    first, runs = None, 0
    for rot in (0, 1, 2, 3, 5, 7, 11, 16):
        order = [(k + rot) % n for k in range(n)]
        for size in (1, 3, 4, 5, n):
            idx = order[:size]
            csr, _ = _rows_of(ctx, [rays[k] for k in idx], 1, flags[idx])
            for j, k in enumerate(idx):
                if first is None and not _same_rows(csr, j, alone[k], 0):
                    first = (rot, size, j, k)
            runs += 1
    envelope["sens/independence"] = {"requests": runs, "first_difference": first}
    assert first is None, first


def test_cut_and_bad_rays(ctx, envelope):
    """MIX_BATCH with its flags: the capacity ray (flag 2; it holds segments whose walk never ends)
    has no entries and status 0, the others the reference's.  A list without flags holding NaN,
    infinite, huge and off-grid points and the never-ending segments (the inputs tests/sens_sim.cpp
    has passed on the host): status 1 and no entries for those, the rays between them the bits they
    have alone."""
    lens, flags, rays = _mix(ctx)
    assert flags[RC.CAP_RAY] == 2 and lens[RC.CAP_RAY] == RC.CAP_POINTS
    m = RC.model(RC.MIX_BATCH.model, RC.MIX_BATCH.nz, RC.MIX_BATCH.nx)
    csr, status = _rows_of(ctx, rays, 1, flags)
    want = SR.rows(_ref_model(m), lens, np.concatenate(rays), 1, RC.DNX, flags)
    _vs_ref(envelope, "cut/mix_batch_flags", csr, status, want)
    assert csr[0][RC.CAP_RAY + 1] == csr[0][RC.CAP_RAY] and not status.any()
    # without its flag the capacity ray is walked: it is invalid (a never-ending segment) or, if all
    # its segments end, has the reference's rows; either way the call returns
    nf = np.zeros_like(flags)
    csr2, status2 = _rows_of(ctx, rays, 1, nf)
    want2 = SR.rows(_ref_model(m), lens, np.concatenate(rays), 1, RC.DNX, nf)
    _vs_ref(envelope, "cut/mix_batch_no_flags", csr2, status2, want2)
    m = RC.model("stripes", *RC.SEG_H)
    RC.set_model(ctx, m)
    for sg in (1, 3):
        ray_len, xy, fl, bad = SR.bad_request(sg)
        _, got, st = ctx.ray_sens(ray_len, xy, subgrid=sg, maps=False, rows=True)  # no flags
        want = SR.rows(_ref_model(m), ray_len, xy, sg, RC.DNX)
        assert np.array_equal(np.nonzero(want[5])[0], bad)
        _vs_ref(envelope, "bad/stripes_sg%d" % sg, got, st, want)
        nrow = np.diff(got[0])
        assert np.all(nrow[bad] == 0) and np.all(st[bad] == 1) and st.sum() == len(bad)
        good, _ = _rows_of(ctx, [xy[0:2]], sg)
        for k in range(0, 2 * len(bad) - 1, 2):
            assert _same_rows(got, k, good, 0), k
        # maps of the same request: the bad rays add nothing, nothing is NaN
        maps, _, st2 = ctx.ray_sens(ray_len, xy, subgrid=sg, maps=True)
        ref, cnt, mag = SR.maps_of(want, m.nz, m.nx)
        assert np.array_equal(st2, st) and np.all(np.isfinite(maps))
        assert np.all(np.abs(maps - ref) <= cnt * MAP * mag)


def _map_check(envelope, name, maps, ref, cnt, mag):
    err = np.abs(maps - ref)
    bound = cnt * MAP * mag
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    envelope["sens/" + name] = {"cells_hit": int(np.count_nonzero(cnt)), "entries_per_cell_max": int(cnt.max()),
                                "err_over_bound_max": ratio, "err_where_no_entries": float(err[:, cnt == 0].max())}
    assert np.all(err <= bound), (name, envelope["sens/" + name])


def test_maps(ctx, envelope):
    """Seeded weights with zeros and negatives: the maps against np.add.at of the reference rows,
    with and without the rows in the same call; rays of weight 0 change nothing."""
    b = [x for x in RC.TRAVEL_BATCHES if x.name == "mixed_41x57_sg3"][0]
    m = RC.model(b.model, b.nz, b.nx)
    RC.set_model(ctx, m)
    for k in range(len(b.fields)):
        ctx.put_field(k, b.sg, RC.field_array(b, k))
    slots = np.array([r[0] for r in b.rays], dtype=np.int32)
    src = np.array([r[1] for r in b.rays], dtype=np.float64)
    rec = np.array([r[2] for r in b.rays], dtype=np.float64)
    t, lens, flags, pts = ctx.find_rays(slots, src, rec, packed=True, check=False)
    n = len(lens)
    rng = np.random.default_rng(5)
    w = rng.normal(size=n)
    w[rng.random(n) < 0.2] = 0.0
    assert np.any(w == 0) and np.any(w < 0) and np.any(w > 0)
    want = SR.rows(_ref_model(m), lens, pts, b.sg, RC.DNX, flags)
    for name, weights in (("weighted", w), ("unit", None)):
        ref, cnt, mag = SR.maps_of(want, b.nz, b.nx, weights)
        only, none, _ = ctx.ray_sens(lens, pts, subgrid=b.sg, flags=flags, weights=weights, maps=True)
        assert none is None
        both, csr, _ = ctx.ray_sens(lens, pts, subgrid=b.sg, flags=flags, weights=weights, maps=True, rows=True)
        _map_check(envelope, "maps/%s_without_rows" % name, only, ref, cnt, mag)
        _map_check(envelope, "maps/%s_with_rows" % name, both, ref, cnt, mag)
        assert np.all(np.abs(only - both) <= 2 * cnt * MAP * mag)
        assert np.array_equal(csr[0], want[0]) and np.array_equal(csr[1], want[1])
    # the coverage map is the sum of the lengths: every ray's length, cell by cell
    ref, cnt, mag = SR.maps_of(want, b.nz, b.nx)
    assert abs(only[0].sum() - want[2].sum()) <= 1e-12 * want[2].sum()
    # weight 0 everywhere: nothing is added
    zero, _, _ = ctx.ray_sens(lens, pts, subgrid=b.sg, flags=flags, weights=np.zeros(n), maps=True)
    assert not zero.any()
    # the zero-weight rays dropped from the request: the same maps within the bound
    live = np.nonzero(w)[0]
    off = np.concatenate(([0], np.cumsum(lens, dtype=np.int64)))
    sub = np.concatenate([pts[off[k]:off[k + 1]] for k in live])
    ref, cnt, mag = SR.maps_of(want, b.nz, b.nx, w)
    fewer, _, _ = ctx.ray_sens(lens[live], sub, subgrid=b.sg, flags=flags[live], weights=w[live], maps=True)
    _map_check(envelope, "maps/zero_weight_rays_dropped", fewer, ref, cnt, mag)


def test_errors(ctx):
    """Every ALIFMM_E_ARG case with its message; the context stays usable."""
    import _alifmm

    L = _alifmm.lib()
    E_ARG = -2
    m = RC.model("stripes", *RC.SEG_H)
    ray_len, xy = SR.segments_request(RC.segments(RC.SEG_H, 1)[:9])
    n = len(ray_len)
    maps = np.zeros((3,) + RC.SEG_H)
    row_ptr = np.zeros(n + 1, dtype=np.int64)

    def call(c, nrays=n, lens=ray_len, pts=xy, mp=None, rp=None, cap=0, arrays=(None, None, None, None), sg=1):
        p = [None if a is None else a.ctypes.data for a in (lens, None, pts, None, mp, rp)]
        q = [None if a is None else a.ctypes.data for a in arrays]
        rc = L.alifmm_ray_sens(c._h, sg, nrays, p[0], p[1], p[2], p[3], p[4], p[5], cap, q[0], q[1], q[2], q[3], None)
        return rc, L.alifmm_last_error(c._h).decode()

    fresh = _alifmm.Context(0)
    try:
        rc, msg = call(fresh, mp=maps)
        assert rc == E_ARG and "no model" in msg, (rc, msg)
    finally:
        fresh.close()
    RC.set_model(ctx, m)
    rc, msg = call(ctx, nrays=-1, mp=maps)
    assert rc == E_ARG and "nrays" in msg, (rc, msg)
    rc, msg = call(ctx, lens=None, mp=maps)
    assert rc == E_ARG and "ray_len" in msg, (rc, msg)
    rc, msg = call(ctx)
    assert rc == E_ARG and "nothing requested" in msg, (rc, msg)
    rc, msg = call(ctx, sg=0, mp=maps)
    assert rc == E_ARG and "subgrid" in msg, (rc, msg)
    col = np.zeros(4096, dtype=np.int32)
    rc, msg = call(ctx, arrays=(col, None, None, None))
    assert rc == E_ARG and "row_ptr" in msg, (rc, msg)
    # the count pass, then a capacity one entry short: E_ARG, row_ptr still holds the sizes
    rc, msg = call(ctx, rp=row_ptr)
    assert rc == 0 and row_ptr[n] > n, (rc, msg)
    total = int(row_ptr[n])
    sizes = row_ptr.copy()
    row_ptr[:] = -1
    col[:] = -7
    rc, msg = call(ctx, rp=row_ptr, cap=total - 1, arrays=(col, None, None, None))
    assert rc == E_ARG and "cap %d < %d" % (total - 1, total) in msg, (rc, msg)
    assert np.array_equal(row_ptr, sizes) and np.all(col == -7)
    # no points kept: NULL points do not add up
    ctx.release_fields()
    rc, msg = call(ctx, pts=None, mp=maps)
    assert rc == E_ARG and "are kept" in msg, (rc, msg)
    # the host-staged keep of a request with two subgrids
    b1, b3 = ([x for x in RC.TRAVEL_BATCHES if x.name == "mixed_41x57_sg%d" % sg][0] for sg in (1, 3))
    RC.set_model(ctx, RC.model(b1.model, b1.nz, b1.nx))
    ctx.put_field(0, 1, RC.field_array(b1, 0))
    ctx.put_field(1, 3, RC.field_array(b3, 0))
    slots = np.array([0, 1], dtype=np.int32)
    src = np.array([b1.rays[0][1], b3.rays[0][1]], dtype=np.float64)
    rec = np.array([b1.rays[0][2], b3.rays[0][2]], dtype=np.float64)
    t2, l2, f2 = np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    assert L.alifmm_find_rays(ctx._h, 2, slots.ctypes.data, src.ctypes.data, rec.ctypes.data, t2.ctypes.data,
                              l2.ctypes.data, f2.ctypes.data, None, _alifmm.KEEP_RAYS) == 0
    mp2 = np.zeros((3, b1.nz, b1.nx))
    rc, msg = call(ctx, nrays=2, lens=l2, pts=None, mp=mp2)
    assert rc == E_ARG and "staged on the host" in msg, (rc, msg)
    ctx.release_fields()
    # still usable
    RC.set_model(ctx, m)
    col = np.zeros(total, dtype=np.int32)
    rc, msg = call(ctx, mp=maps, rp=row_ptr, cap=total, arrays=(col, None, None, None))
    assert rc == 0 and np.array_equal(row_ptr, sizes) and maps[0].sum() > 0, (rc, msg)


def test_dropin_ray_sensitivity(envelope):
    """ALI_FMM.ray_sensitivity on a 41 x 57 grain model, 4 transducers, rays at subgrid 3: its maps
    equal the Context path's within the map bound, and the per-ray sums of the CSR's time entries
    match the times matrix of find_all_TTF_rays."""
    import Anis_TTF_rays as A

    m = RC.model("grain", 41, 57)
    veln, velpn, vm, sd = (np.array(a) for a in (m.veln, m.velpn, m.vm, m.sd))
    scx = RC.DNX * np.array([5.0, 20.0, 36.0, 51.0])
    scz = RC.DNX * np.array([0.0, 40.0, 40.0, 0.0])
    M = A.ALI_FMM(veln, velpn, vm, scx, scz, stif_den=sd, dnx=RC.DNX)
    times = M.find_all_TTF_rays(veln, velpn, vm, subgrid_size=3, stif_den=sd)
    w = np.random.default_rng(9).normal(size=(4, 4))
    maps, csr, pairs = M.ray_sensitivity(weights=w, rows=True)
    assert maps.shape == (3, 41, 57) and len(pairs) == 6
    worst = 0.0
    for k, (i, j) in enumerate(pairs):
        s = float(np.sum(csr[3][csr[0][k]:csr[0][k + 1]]))
        worst = max(worst, abs(s - times[i, j]) / times[i, j])
    envelope["sens/dropin/time_sum_rel_max"] = worst
    assert worst <= EXACT, worst
    # the Context path on the stored points
    store = M.rays
    lens = store.ray_len[pairs[:, 0], pairs[:, 1]]
    pts = np.concatenate([np.stack(store.path(i, j), axis=1) for i, j in pairs])
    cmaps, ccsr, status = M._ctx(0).ray_sens(lens, pts, subgrid=1, weights=w[pairs[:, 0], pairs[:, 1]], maps=True, rows=True)
    assert not status.any() and all(np.array_equal(a, b) for a, b in zip(csr, ccsr))
    ref, cnt, mag = SR.maps_of(ccsr + (status,), 41, 57, w[pairs[:, 0], pairs[:, 1]])
    _map_check(envelope, "dropin/maps_vs_rows", maps, ref, cnt, mag)
    _map_check(envelope, "dropin/context_maps_vs_rows", cmaps, ref, cnt, mag)
    one = M.ray_sensitivity(pairs=[(0, 1)])  # maps only, one ray, unit weight
    assert abs(one[1].sum() - times[0, 1]) <= 1e-12 * times[0, 1]
