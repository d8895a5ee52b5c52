"""The ray tracer (csrc/rays.hip find_ray_kernel / tbp_wave, utils.hip tbp_kernel, host_rays.cpp
alifmm_find_rays) against the CPU oracle on the small-shape matrix of tests/ray_cases.py.  Every
field is uploaded (alifmm_put_field), so the ray kernel runs on exactly known fields, independent of
the band kernel.  Run on the GPU box: pytest -m gpu.

Reference and bars: the correctly rounded build of the oracle (oracle/lib/liboracle_cr.so, the
device's trigonometry) on the same field, at the project's bars for rays on a given field
(tests/test_gpu_parity.py): lengths and flags equal, points <= 1e-9, times <= 1e-12 relative.  On the
oracle's return codes -3 (point capacity) and -4 (empty search plane) the device must set flag 2 / 4
and hold the points walked so far; on the early exit flag 1 and the whole ray.
tests/test_oracle.py::test_ray_case_matrix_preconditions holds everything that is taken from the
oracle alone (case classes, agreement of the glibc and the correctly rounded build).  The worst
values and the bit-exact fractions of every group go to the session's parity envelope under
"rays_small/..." before anything is asserted.

What each group covers:
  * segments[model]: ~270 single segments per subgrid (1: 16-lane groups, 3: 32-lane) through
    tbp_wave in the kernel's ray_time loop and through tbp_kernel: node-to-node segments of 1 .. 256
    nodes in both directions and both axes, 8 / 9 pieces (the read-ahead), 12 / 13 pieces (the kept
    lengths), 1, 2, 4, 5, 9 and 10 runs (kRuns 4: more take the one-lane loop), a run starting at
    piece 7, 8, 11, 12 and 256 (piece indices past 255 force the one-lane loop), A B A, exact
    diagonals, the grid's first and last row and column, zero length, 200 seeded oblique segments.
    Models iso, stripes, mixed (200 records), m256 (material id 255): LDSMAT = true; m257 (nmat 257),
    stif65 (65 stiffness rows) and vt3 (3-column table, velpn 0 / 1 / 2): LDSMAT = false.
  * walks[batch]: whole rays on oracle fields (grain, mixed; 41 x 57, 57 x 41; subgrid 1: 16
    lanes, 3: 32 lanes), on synthetic fields at subgrid 5, 9 (64 lanes) and 11 (69 candidates: the
    candidate loop's second round), on a 2-row and a 3-column grid, the diagonal-plane .5 ties
    (rec_TTF read off the search plane), and one case per exit of the walk at every subgrid: early
    exit (flag 1), axis plane leaving the grid, empty plane (flag 4), loop not entered.
  * nine_lanes: a request that fills the device (9-lane groups, two launches, points kept) equals
    the 16-lane request tile by tile; last wavefronts with 1 and 6 of their 7 groups.
  * independence: 2-point rays, the 610-point capacity ray (flag 2), an early exit and ordinary
    rays on three fields in one list, rotated and cut to 1, 3, 4, 5, 15, 16, 17 rays: every ray has
    the same bits whatever its slot and neighbours, equal to the ray run alone.
  * mixed_subgrids, direct_buffer: the host paths of alifmm_find_rays (by_sg grouping with
    host-staged points, the caller's ray_xy buffer and its capacity error).

Different fields per ray in one wavefront: the segment groups (up to 48 pit fields, 4 rays per
wavefront) and the independence list (three slots interleaved, each repeated).

Measured on the MI355X when the file was written: every group 100 % bit-exact, times and points
(time_rel_max 0, point_err_max 0), tbp_kernel 100 % bit-equal to the oracle and to the ray kernel's
segment times; the bars stay where the project has them.

Bug found by the matrix and fixed with it (rays.hip): the kernel ran its ray_time loop over rays it
had cut short (flag 2 or 4).  The reference raises there and never times such a ray, and the
capacity ray circling the ring holds horizontal segments at z = k + 0.5 (k odd) for which
time_between_points()'s walk has next_y == end_y at its start, never sets fin_y and runs off the
grid without end (ray_cases.walk_cells): the kernel read material ids out of bounds, an illegal
memory access.  A ray cut short now has time 0 (include/alifmm.h).
"""
import ctypes

import numpy as np
import pytest

import oracle as O
import ray_cases as RC

pytestmark = pytest.mark.gpu

EXACT = 1e-12  # times, relative (tests/test_gpu_parity.py)
POINTS = 1e-9  # points, fine-grid nodes
REF = O.LIB_CR
LANES = {1: 16, 3: 32, 5: 64, 9: 64, 11: 64}


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    yield c
    c.close()


def _upload(c, b, first=0):
    for k in range(len(b.fields)):
        c.put_field(first + k, b.sg, RC.field_array(b, k))


def _request(b, idx=None, first=0):
    rays = b.rays if idx is None else [b.rays[k] for k in idx]
    return (np.array([first + r[0] for r in rays], dtype=np.int32), np.array([r[1] for r in rays], dtype=np.float64),
            np.array([r[2] for r in rays], dtype=np.float64))


def _trace(c, b, idx=None, first=0, check=False):
    """(times, lens, flags, list of (n, 2) point arrays) of rays `idx` of a batch."""
    slots, src, rec = _request(b, idx, first)
    t, lens, flags, pts = c.find_rays(slots, src, rec, packed=True, check=check)
    off = np.concatenate(([0], np.cumsum(lens, dtype=np.int64)))
    return t, lens, flags, [pts[off[k]:off[k + 1]] for k in range(len(lens))]


def _vs_oracle(envelope, group, b, got, refs=None, extra=None):
    """Every ray of a batch against the oracle's; the figures are recorded before anything is
    asserted."""
    t, lens, flags, rays = got
    refs = RC.batch_reference(b, REF) if refs is None else refs
    assert len(refs) == len(t)
    bad = []
    t_rel = p_err = 0.0
    t_exact = t_n = p_exact = p_n = 0
    for k, r in enumerate(refs):
        want_len = r.rc if r.rc >= 0 else r.walked + 1
        want_flag = {-3: 2, -4: 4}.get(r.rc, r.early)
        if int(lens[k]) != want_len or int(flags[k]) != want_flag:
            bad.append((k, "len/flag", int(lens[k]), int(flags[k]), want_len, want_flag))
            continue
        p = rays[k]
        ox, oy = r.x, r.y
        if r.rc < 0:  # the walked points, then the receiver
            if tuple(p[-1]) != tuple(b.rays[k][2]):
                bad.append((k, "receiver", tuple(p[-1])))
            if t[k] != 0.0:  # a ray cut short is not timed (include/alifmm.h)
                bad.append((k, "time of a cut ray", float(t[k])))
            p = p[:-1]
        e = max(float(np.max(np.abs(p[:, 0] - ox))), float(np.max(np.abs(p[:, 1] - oy))))
        p_err = max(p_err, e)
        p_exact += int(np.sum(p[:, 0] == ox)) + int(np.sum(p[:, 1] == oy))
        p_n += 2 * len(ox)
        if not e <= POINTS:
            bad.append((k, "points", e))
        if r.rc >= 0:
            rel = abs(t[k] - r.t) / r.t if r.t != 0 else abs(t[k])
            t_rel = max(t_rel, float(rel))
            t_exact += int(t[k] == r.t)
            t_n += 1
            if not rel <= EXACT:
                bad.append((k, "time", float(t[k]), r.t))
    rec = {"rays": len(refs), "time_rel_max": t_rel, "time_exact_frac": t_exact / max(t_n, 1),
           "point_err_max": p_err, "point_exact_frac": p_exact / max(p_n, 1), "mismatches": len(bad)}
    rec.update(extra or {})
    envelope["rays_small/" + group] = rec
    assert not bad, (group, bad[:5], rec)
    return rec


def _same(a, b, ia=None, ib=None):
    """Rays ia of result a and ib of result b: the same bits (times, lengths, flags, points)."""
    ia = range(len(a[0])) if ia is None else ia
    ib = range(len(b[0])) if ib is None else ib
    for i, j in zip(ia, ib):
        if not (a[0][i] == b[0][j] and a[1][i] == b[1][j] and a[2][i] == b[2][j] and np.array_equal(a[3][i], b[3][j])):
            return (i, j, a[0][i], b[0][j], int(a[1][i]), int(b[1][j]), int(a[2][i]), int(b[2][j]))
    return None


def _fill9(c):
    """Rays from which a request gets 9-lane groups (host_rays.cpp alifmm_find_rays fill9)."""
    return int(c.get_option("n_cu")) * 4 * int(c.get_option("ray_waves_per_simd")) * 7


@pytest.mark.parametrize("mname,shape", RC.SEGMENT_RUNS, ids=["%s_%dx%d" % (m, s[0], s[1]) for m, s in RC.SEGMENT_RUNS])
def test_segments(ctx, envelope, mname, shape):
    """Single segments through the ray kernel (2-point rays on pit fields) and through tbp_kernel,
    against the oracle's ray and time_between_points of the same segment."""
    m = RC.model(mname, *shape)
    RC.set_model(ctx, m)
    count, lds = RC.SEG_MODELS[mname]
    nmat = int(ctx.get_option("nmat"))
    assert nmat == RC.record_count(m), (mname, nmat)
    # af_launch_rays' condition for the LDS tables (nmat <= 256, <= 64 stiffness rows, 361 ncol <= 722)
    assert lds == (nmat <= 256 and RC.stiffness_rows(m) <= 64 and 361 * m.table.shape[1] <= 722)
    for sg in RC.SEG_SUBGRIDS:
        b = RC.segment_batch(mname, shape, sg)
        _upload(ctx, b)
        got = _trace(ctx, b)
        assert ctx.get_option("ray_lanes") == LANES[sg]
        segs = RC.segments(shape, sg)
        x1, y1, x2, y2 = (np.array([getattr(s, f) for s in segs]) for f in ("x1", "y1", "x2", "y2"))
        tk = ctx.time_between_points(x1, x2, y1, y2, sg)
        want = RC.segment_times(mname, shape, sg, REF)
        rel = np.abs(tk - want) / np.where(want != 0, want, 1.0)
        name = "segments/%s_%dx%d_sg%d" % (mname, shape[0], shape[1], sg)
        keep = RC.ray_segments(shape, sg)[0]
        _vs_oracle(envelope, name, b, got,
                   extra={"lds": lds, "tbp_kernel_rel_max": float(rel.max()), "tbp_kernel_exact_frac": float(np.mean(tk == want)),
                          "ray_kernel_equals_tbp_kernel_frac": float(np.mean(got[0] == tk[keep]))})
        assert np.all(got[1] == 2)
        assert rel.max() <= EXACT, (name, segs[int(np.argmax(rel))].name, float(rel.max()))


WALKS = RC.WALK_BATCHES + [RC.DIAG_TIE_BATCH] + RC.EXIT_BATCHES


@pytest.mark.parametrize("b", WALKS, ids=[b.name for b in WALKS])
def test_walks(ctx, envelope, b):
    """Whole rays on uploaded fields, per subgrid and lane count, and every exit of the walk."""
    import _alifmm

    RC.set_model(ctx, RC.model(b.model, b.nz, b.nx))
    _upload(ctx, b)
    got = _trace(ctx, b)
    assert ctx.get_option("ray_lanes") == LANES[b.sg]
    _vs_oracle(envelope, "walks/" + b.name, b, got)
    if any(r.rc == -4 for r in RC.batch_reference(b, REF)):
        with pytest.raises(_alifmm.AlifmmError, match="empty plane-search"):
            _trace(ctx, b, check=True)


def test_nine_lanes_and_kept_points_across_launches(ctx, envelope):
    """A request of n_cu * 4 * waves per SIMD * 7 + 5 rays made by tiling a walk batch: 9-lane
    groups, two launches, the kept points equal the small (16-lane) request's tile by tile."""
    b = [x for x in RC.TRAVEL_BATCHES if x.name == "mixed_41x57_sg1"][0]
    RC.set_model(ctx, RC.model(b.model, b.nz, b.nx))
    _upload(ctx, b)
    small = _trace(ctx, b)
    assert ctx.get_option("ray_lanes") == 16
    n = len(b.rays)
    big = _fill9(ctx) + 5
    idx = [k % n for k in range(big)]
    got = _trace(ctx, b, idx)
    assert ctx.get_option("ray_lanes") == 9
    diff = _same(got, small, range(big), idx)
    envelope["rays_small/nine_lanes"] = {"rays": big, "first_difference": diff}
    assert diff is None, diff
    _vs_oracle(envelope, "nine_lanes_vs_oracle", b, tuple(v[:n] for v in got))


def test_position_and_batch_independence(ctx, envelope):
    """One list of 2-point rays, the capacity ray, an early exit and ordinary rays on three fields,
    in rotations and at request sizes around a wavefront's 4 groups (and, within 9-lane requests,
    with 1 and with 6 of the last wavefront's 7 groups): every ray has the same bits whatever its
    slot and neighbours, and equals the ray run alone; check=True raises for the capacity ray."""
    import _alifmm

    b = RC.MIX_BATCH
    RC.set_model(ctx, RC.model(b.model, b.nz, b.nx))
    _upload(ctx, b)
    n = len(b.rays)
    alone = [_trace(ctx, b, [k]) for k in range(n)]
    alone = tuple([a[f][0] for a in alone] for f in range(4))
    rec = _vs_oracle(envelope, "independence/alone", b, alone)
    assert int(alone[1][RC.CAP_RAY]) == RC.CAP_POINTS and int(alone[2][RC.CAP_RAY]) == 2
    with pytest.raises(_alifmm.RayCapacityError):
        _trace(ctx, b, check=True)
    runs = 0
    first = None
    for rot in (0, 1, 2, 3, 5, 7, 11, 16):
        order = [(k + rot) % n for k in range(n)]
        for size in (1, 3, 4, 5, 15, 16, 17):
            idx = order[:size]
            d = _same(_trace(ctx, b, idx), alone, range(size), idx)
            first = first or (d and (rot, size) + d)
            runs += 1
    # 9-lane requests (two launches each): chunks of 7 a + 1 and 7 a + 6 rays
    fill = _fill9(ctx)
    for last in (1, 6):
        big = next(m for m in range(fill + 1, fill + 40) if ((m + 1) // 2) % 7 == last)
        idx = [(3 * k + last) % n for k in range(big)]
        got = _trace(ctx, b, idx)
        assert ctx.get_option("ray_lanes") == 9
        d = _same(got, alone, range(big), idx)
        first = first or (d and ("nine", big) + d)
        runs += 1
    envelope["rays_small/independence"] = {"requests": runs, "first_difference": first, "alone": rec}
    assert first is None, first


def test_mixed_subgrids_in_one_call(ctx, envelope):
    """Slots of subgrid 1 and 3 interleaved in one request (alifmm_find_rays' by_sg grouping and
    host-staged points): times, lengths, flags and packed points come back in the caller's order and
    equal the per-subgrid calls."""
    b1, b3 = ([x for x in RC.TRAVEL_BATCHES if x.name == "mixed_41x57_sg%d" % sg][0] for sg in (1, 3))
    RC.set_model(ctx, RC.model(b1.model, b1.nz, b1.nx))
    _upload(ctx, b1, 0)
    _upload(ctx, b3, len(b1.fields))
    one = _trace(ctx, b1)
    three = _trace(ctx, b3, first=len(b1.fields))
    r1, r3 = _request(b1), _request(b3, first=len(b1.fields))
    n = len(b1.rays)
    assert len(b3.rays) == n
    # a seeded shuffle of both lists: neither group is a stride of the request or keeps its order
    order = [(int(j) // n, int(j) % n) for j in np.random.default_rng(5).permutation(2 * n)]
    slots = np.array([(r1, r3)[w][0][k] for w, k in order], dtype=np.int32)
    src = np.array([(r1, r3)[w][1][k] for w, k in order])
    rec = np.array([(r1, r3)[w][2][k] for w, k in order])
    t, lens, flags, pts = ctx.find_rays(slots, src, rec, packed=True)
    off = np.concatenate(([0], np.cumsum(lens, dtype=np.int64)))
    got = (t, lens, flags, [pts[off[k]:off[k + 1]] for k in range(2 * n)])
    first = None
    for j, (w, k) in enumerate(order):
        first = first or _same(got, (one, three)[w], [j], [k])
    envelope["rays_small/mixed_subgrids"] = {"rays": 2 * n, "first_difference": first}
    assert first is None, first
    at = [order.index((1, k)) for k in range(n)]  # the subgrid-3 rays, back in their batch's order
    _vs_oracle(envelope, "mixed_subgrids_sg3_vs_oracle", b3, tuple([got[f][j] for j in at] for f in range(4)))


def test_direct_output_buffer(ctx, envelope):
    """alifmm_find_rays with the caller's ray_xy buffer (the binding always keeps the points in the
    context instead): the same layout and bits as KEEP_RAYS + take_rays; a capacity one point short
    is ALIFMM_E_ARG with its message, take_rays then reports 0 kept points, and the next call on the
    same context succeeds."""
    import _alifmm

    L = _alifmm.lib()
    b1, b3 = ([x for x in RC.TRAVEL_BATCHES if x.name == "mixed_41x57_sg%d" % sg][0] for sg in (1, 3))
    RC.set_model(ctx, RC.model(b1.model, b1.nz, b1.nx))
    _upload(ctx, b1, 0)
    _upload(ctx, b3, len(b1.fields))
    r1, r3 = _request(b1), _request(b3, first=len(b1.fields))
    both = tuple(np.ascontiguousarray(np.concatenate([a, c])[::-1]) for a, c in zip(r1, r3))  # subgrid 3 first
    checked = 0
    for slots, src, rec in (r1, both):
        n = len(slots)
        tk, lk, fk, pk = ctx.find_rays(slots, src, rec, packed=True)
        npts = len(pk)

        def direct(cap):
            t, ln, fl = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
            xy = np.full((max(cap, 1) + 1, 2), -7.0)  # one guard row past the capacity
            rc = L.alifmm_find_rays(ctx._h, n, slots.ctypes.data, src.ctypes.data, rec.ctypes.data, t.ctypes.data,
                                    ln.ctypes.data, fl.ctypes.data, xy.ctypes.data, cap)
            return rc, t, ln, fl, xy

        rc, t, ln, fl, xy = direct(npts)
        assert rc == 0
        assert np.array_equal(t, tk) and np.array_equal(ln, lk) and np.array_equal(fl, fk)
        assert np.array_equal(xy[:npts], pk) and np.all(xy[npts:] == -7.0)
        rc, t, ln, fl, xy = direct(npts - 1)
        assert rc == -2  # ALIFMM_E_ARG
        msg = L.alifmm_last_error(ctx._h).decode()
        assert "ray_xy capacity %d < %d" % (npts - 1, npts) in msg, msg
        assert np.all(xy == -7.0)  # no point written into the short buffer
        got = ctypes.c_int64(-1)
        assert L.alifmm_take_rays(ctx._h, None, 0, ctypes.byref(got)) == 0 and got.value == 0
        rc, t, ln, fl, xy = direct(npts)
        assert rc == 0 and np.array_equal(t, tk) and np.array_equal(xy[:npts], pk)
        tk2, lk2, fk2, pk2 = ctx.find_rays(slots, src, rec, packed=True)
        assert np.array_equal(tk2, tk) and np.array_equal(pk2, pk)
        checked += n
    envelope["rays_small/direct_buffer"] = {"rays": checked, "bit_identical": True}
