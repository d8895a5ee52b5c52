"""Back-wall echo paths between element pairs on the device (csrc/skip_pairs.hip, host_rays.cpp
alifmm_skip_pick / alifmm_skip_rays, Context.skip_pick / skip_rays, ALI_FMM.find_all_skip_rays)
against the numpy restatement tests/skip_ref.py, the host composition of two alifmm_find_rays calls,
the CPU oracle and tests/sens_ref.py.  Fields are uploaded (alifmm_put_field) wherever the bits
matter, so the kernels run on exactly known fields.  Run on the GPU box: pytest -m gpu.

Bars: the pick and the join are bit for bit (they add two doubles and move points); the legs meet
the project's bars for rays on a given field (tests/test_gpu_rays_small.py: lengths and flags equal,
points <= 1e-9, times <= 1e-12 relative), the rows those of tests/test_gpu_sens.py.  The figures go
to the session's parity envelope under "skip_pairs/..." before anything is asserted.
"""
import ctypes

import numpy as np
import pytest

import ray_cases as RC
import sens_ref as SR
import skip_ref as S

pytestmark = pytest.mark.gpu

EXACT = 1e-12  # times, relative
POINTS = 1e-9  # points, fine-grid nodes
DTH = 2.0 ** -40
NWS = (1, 63, 64, 65, 255, 257, 1000)
NPAIRS = (1, 7, 300)


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _case(name):
    return [c for c in S.CASES if c.name == name][0]


def _upload(ctx, c, first=0):
    RC.set_model(ctx, RC.model(c.model, c.nz, c.nx))
    F = S.fields(c)
    for k in range(len(F)):
        ctx.put_field(first + k, c.sg, F[k])
    return F


def _reflectors(c, rng):
    """name -> (w_iz, w_ix): the last row, shuffled subsets of it, a column, scattered nodes with
    repeats at every size of NWS."""
    fz, fx = c.sg * (c.nz - 1) + 1, c.sg * (c.nx - 1) + 1
    row = S.back_wall(c)
    out = {"last_row": row}
    for nw in NWS:
        if nw <= fx:
            keep = rng.permutation(fx)[:nw].astype(np.int32)
            out["row_subset_%d" % nw] = (row[0][:nw].copy(), keep)
        iz = rng.integers(0, fz, nw).astype(np.int32)
        ix = rng.integers(0, fx, nw).astype(np.int32)
        iz[nw // 2:], ix[nw // 2:] = iz[:nw - nw // 2], ix[:nw - nw // 2]  # every node of the first half again
        out["scattered_%d" % nw] = (iz, ix)
    out["column"] = (np.arange(fz, dtype=np.int32), np.full(fz, fx // 3, dtype=np.int32))
    return out


@pytest.mark.parametrize("sg", [1, 3])
def test_pick_bits(ctx, envelope, sg):
    """hit and pick_time equal numpy's on the same arrays bit for bit, for every reflector kind and
    size and every request size, with repeated slots and a = b; one pair has the same bits at every
    position and request size."""
    c = _case("grain_41x57_sg%d" % sg)
    first = 3
    F = _upload(ctx, c, first)
    rng = np.random.default_rng(40 + sg)
    checked = 0
    bad = []
    for name, (w_iz, w_ix) in _reflectors(c, rng).items():
        probe = None
        for n in NPAIRS:
            a = rng.integers(0, S.NELEM, n).astype(np.int32)
            b = rng.integers(0, S.NELEM, n).astype(np.int32)
            a[n // 2], b[n // 2] = 1, 4            # the probe pair, somewhere else in every request
            if n > 2:
                a[0] = b[0] = 2                    # a = b
            pt, hit = ctx.skip_pick(first + a, first + b, w_iz, w_ix)
            wpt, whit = S.pick(F, a, b, w_iz, w_ix)
            if not (np.array_equal(hit, whit) and _same_bits(pt, wpt)):
                bad.append((name, n, int(np.argmax((hit != whit) | (_bits(pt) != _bits(wpt))))))
            p = (int(hit[n // 2]), float(pt[n // 2]))
            probe = probe or p
            if p != probe:
                bad.append((name, n, "probe", p, probe))
            checked += n
    envelope["skip_pairs/pick_bits/sg%d" % sg] = {"pairs": checked, "mismatches": len(bad), "first": bad[:3]}
    assert not bad, bad[:5]
    assert ctx.get_option("skip_pick_ms") > 0


def test_pick_crafted_fields(ctx, envelope):
    """Equal least sums give the lower node number; NaN and +-inf nodes are skipped; a pair with no
    finite node gives -1 and +inf and leaves its neighbours in the request as they are."""
    c = _case("grain_41x57_sg1")
    RC.set_model(ctx, RC.model(c.model, c.nz, c.nx))
    fz, fx = c.nz, c.nx
    rng = np.random.default_rng(9)
    F = np.empty((5, fz, fx))
    F[0] = rng.integers(8, 40, (fz, fx)) / 8.0
    F[1] = rng.integers(8, 40, (fz, fx)) / 8.0
    F[2] = F[0]
    F[2][rng.random((fz, fx)) < 0.3] = np.nan
    F[2][rng.random((fz, fx)) < 0.2] = np.inf
    F[2][rng.random((fz, fx)) < 0.2] = -np.inf
    F[3] = np.nan
    F[4] = 0.0
    w_iz, w_ix = S.back_wall(c)
    # two nodes with the same least sum, the lower one later in a lane's stride than the higher is early
    F[0][fz - 1, :] = 5.0
    F[0][fz - 1, 50] = F[0][fz - 1, 7] = 0.25
    F[4][fz - 1, 3] = -np.inf
    for k in range(5):
        ctx.put_field(k, 1, F[k])
    a = np.array([0, 0, 3, 2, 0, 3, 4, 2, 1, 3], dtype=np.int32)
    b = np.array([4, 0, 0, 2, 1, 3, 4, 1, 1, 4], dtype=np.int32)
    pt, hit = ctx.skip_pick(a, b, w_iz, w_ix)
    wpt, whit = S.pick(F, a, b, w_iz, w_ix)
    alone = [ctx.skip_pick(a[k:k + 1], b[k:k + 1], w_iz, w_ix) for k in range(len(a))]
    rec = {"hit": hit.tolist(), "want": whit.tolist(), "no_hit_pairs": int(np.sum(whit < 0))}
    envelope["skip_pairs/pick_crafted"] = rec
    assert np.array_equal(hit, whit) and _same_bits(pt, wpt), rec
    assert hit[0] == 7 and pt[0] == 0.25 and hit[1] == 7 and pt[1] == 0.5
    assert list(hit[[2, 5, 9]]) == [-1, -1, -1] and np.all(np.isposinf(pt[[2, 5, 9]]))
    assert hit[3] >= 0 and np.isfinite(F[2][w_iz[hit[3]], w_ix[hit[3]]])
    assert hit[6] == 0  # -inf at node 3 is no candidate; all others tie at 0.0
    for k in range(len(a)):
        assert alone[k][1][0] == hit[k] and _same_bits(alone[k][0], pt[k:k + 1])


def _legs_on_device(ctx, c, sa, sb, a_xy, b_xy, w_iz, w_ix, hit, first):
    """Two find_rays calls (the legs to a, the legs to b) for the pairs with a hit -> S.compose input."""
    live = np.nonzero(hit >= 0)[0]
    src = np.stack([w_ix[hit[live]], w_iz[hit[live]]], axis=1).astype(np.float64)
    out = [None] * len(hit)
    res = []
    for s, xy in ((sa, a_xy), (sb, b_xy)):
        t, ln, fl, pts = ctx.find_rays(first + s[live], src, xy[live], packed=True, check=False)
        off = np.concatenate(([0], np.cumsum(ln, dtype=np.int64)))
        res.append([(float(t[i]), int(ln[i]), int(fl[i]), pts[off[i]:off[i + 1]]) for i in range(len(live))])
    for i, k in enumerate(live):
        out[k] = (res[0][i], res[1][i])
    return out


def _raw_skip_rays(ctx, sa, sb, a_xy, b_xy, w_iz, w_ix, cap):
    """alifmm_skip_rays with the caller's ray_xy buffer (one guard row past the capacity)."""
    import _alifmm

    L = _alifmm.lib()
    n = len(sa)
    pt, hit = np.full(n, -5.0), np.full(n, -5, dtype=np.int32)
    t, ln, fl = np.full(n, -5.0), np.full(n, -5, dtype=np.int32), np.full(n, -5, dtype=np.int32)
    xy = np.full((max(cap, 1) + 1, 2), -7.0)
    sa, sb = np.ascontiguousarray(sa, dtype=np.int32), np.ascontiguousarray(sb, dtype=np.int32)
    a_xy, b_xy = np.ascontiguousarray(a_xy), np.ascontiguousarray(b_xy)
    rc = L.alifmm_skip_rays(ctx._h, n, sa.ctypes.data, sb.ctypes.data, a_xy.ctypes.data, b_xy.ctypes.data, len(w_iz),
                            w_iz.ctypes.data, w_ix.ctypes.data, pt.ctypes.data, hit.ctypes.data, t.ctypes.data,
                            ln.ctypes.data, fl.ctypes.data, xy.ctypes.data, cap)
    return rc, pt, hit, t, ln, fl, xy


def _rows_vs_ref(got, status, want):
    """The bars of tests/test_gpu_sens.py for a request's rows; returns the figures."""
    rec = {"counts_equal": bool(np.array_equal(got[0], want[0])), "status_equal": bool(np.array_equal(status, want[5]))}
    if rec["counts_equal"]:
        t_ref = want[3]
        rel = np.abs(got[3] - t_ref) / np.where(t_ref != 0, np.abs(t_ref), 1.0)
        rec.update({"col_equal": bool(np.array_equal(got[1], want[1])), "len_equal": bool(np.array_equal(got[2], want[2])),
                    "time_rel_max": float(rel.max()), "dth_ok": bool(np.all(np.abs(got[4] - want[4]) <= DTH * np.abs(t_ref)))})
    return rec


@pytest.mark.parametrize("c", S.CASES, ids=[c.name for c in S.CASES])
def test_rays(ctx, envelope, c):
    """The 15 pairs of a case on uploaded oracle fields, with one pair that has no hit in their midst."""
    import _alifmm

    L = _alifmm.lib()
    first = 2
    F = _upload(ctx, c, first)
    dead = first + S.NELEM  # a field of NaN: no node has a finite sum with it
    ctx.put_field(dead, c.sg, np.full(F[0].shape, np.nan))
    sa, sb, a_xy, b_xy = S.request(c)
    w_iz, w_ix = S.back_wall(c)
    comp = S.oracle_composition(c)
    n = len(sa)
    rec = {"pairs": n}
    # 1. the joined rays against the host composition of two find_rays calls, bit for bit
    pt, hit, t, ln, fl, pts = ctx.skip_rays(first + sa, first + sb, a_xy, b_xy, w_iz, w_ix, check=False)
    assert ctx.get_option("ray_lanes") == {1: 16, 3: 32}[c.sg]
    join_ms, ray_ms = ctx.get_option("skip_join_ms"), ctx.get_option("ray_kernel_ms")
    legs = _legs_on_device(ctx, c, sa, sb, a_xy, b_xy, w_iz, w_ix, hit, first)
    wt, wln, wfl, wpts = S.compose(hit, legs)
    rec["pick_equals_restatement"] = bool(np.array_equal(hit, comp.hit) and _same_bits(pt, comp.pick))
    rec["joined_equals_two_find_rays"] = bool(_same_bits(t, wt) and np.array_equal(ln, wln) and np.array_equal(fl, wfl)
                                              and _same_bits(pts, np.concatenate(wpts)))
    # 2. the legs against the oracle's
    p_err = t_rel = 0.0
    legs_ok = True
    for k in range(n):
        for (lt, ll, lf, lp), r in zip(legs[k], comp.legs[k]):
            if r.rc <= 0 or ll != r.rc or lf != r.early:
                legs_ok = False
                continue
            p_err = max(p_err, float(np.max(np.abs(lp[:, 0] - r.x))), float(np.max(np.abs(lp[:, 1] - r.y))))
            t_rel = max(t_rel, abs(lt - r.t) / r.t)
    rec.update({"legs_len_flags_equal": legs_ok, "leg_point_err_max": p_err, "leg_time_rel_max": t_rel})
    # 3. the caller's buffer against the kept points
    npts = len(pts)
    rc, pt2, hit2, t2, ln2, fl2, xy = _raw_skip_rays(ctx, first + sa, first + sb, a_xy, b_xy, w_iz, w_ix, npts)
    rec["buffer_equals_kept"] = bool(rc == 0 and _same_bits(xy[:npts], pts) and np.all(xy[npts:] == -7.0)
                                     and _same_bits(t2, t) and np.array_equal(ln2, ln) and np.array_equal(fl2, fl)
                                     and np.array_equal(hit2, hit) and _same_bits(pt2, pt))
    # 4. rows: the kept joined rays read in place, the same points from the host, the restatement
    r5 = ctx.skip_rays(first + sa, first + sb, a_xy, b_xy, w_iz, w_ix, with_points="keep", check=False)
    _, dev, dstat = ctx.ray_sens(ln, None, subgrid=c.sg, flags=fl, maps=False, rows=True)
    got = ctypes.c_int64(-1)
    back = np.empty_like(pts)
    took = L.alifmm_take_rays(ctx._h, back.ctypes.data, len(back), ctypes.byref(got))
    _, host, hstat = ctx.ray_sens(ln, pts, subgrid=c.sg, flags=fl, maps=False, rows=True)
    want = SR.rows(SR.Model(RC.model(c.model, c.nz, c.nx)), ln, pts, c.sg, RC.DNX, fl)
    rec["kept_still_there_after_sens"] = bool(took == 0 and got.value == npts and _same_bits(back, pts)
                                              and np.array_equal(r5[3], ln))
    rec["rows_kept_equal_host"] = bool(all(_same_bits(dev[q], host[q]) for q in range(5)) and np.array_equal(dstat, hstat))
    rec["rows"] = _rows_vs_ref(host, hstat, want)
    row_sum = max(abs(float(np.sum(host[3][host[0][k]:host[0][k + 1]])) - t[k]) / t[k] for k in range(n))
    rec["row_time_sum_vs_times_rel_max"] = row_sum
    # 5. a pair without a hit in the request: empty, flag 8, no rows; the others unchanged
    at = 7
    sa3, sb3 = np.insert(first + sa, at, first + 1), np.insert(first + sb, at, dead)
    a3, b3 = np.insert(a_xy, at, a_xy[1], axis=0), np.insert(b_xy, at, b_xy[1], axis=0)
    pt3, hit3, t3, ln3, fl3, pts3 = ctx.skip_rays(sa3, sb3, a3, b3, w_iz, w_ix, check=False)
    others = np.arange(n + 1) != at
    rec["no_hit_pair"] = bool(hit3[at] == -1 and np.isposinf(pt3[at]) and ln3[at] == 0 and fl3[at] == 8 and t3[at] == 0.0)
    rec["no_hit_others_unchanged"] = bool(np.array_equal(hit3[others], hit) and _same_bits(t3[others], t)
                                          and np.array_equal(ln3[others], ln) and np.array_equal(fl3[others], fl)
                                          and _same_bits(pts3, pts))
    ctx.skip_rays(sa3, sb3, a3, b3, w_iz, w_ix, with_points="keep", check=False)
    _, dev3, dstat3 = ctx.ray_sens(ln3, None, subgrid=c.sg, flags=fl3, maps=False, rows=True)
    rec["no_hit_no_rows"] = bool(dev3[0][at] == dev3[0][at + 1] and dstat3[at] == 0 and dev3[0][-1] == host[0][-1]
                                 and all(_same_bits(dev3[q], host[q]) for q in range(1, 5)))
    rec["join_ms"], rec["ray_kernel_ms"] = join_ms, ray_ms
    envelope["skip_pairs/rays/" + c.name] = rec
    assert rec["pick_equals_restatement"] and rec["joined_equals_two_find_rays"], rec
    assert np.array_equal(fl, comp.flags) and np.array_equal(ln, comp.lens), rec
    assert legs_ok and p_err <= POINTS and t_rel <= EXACT, rec
    assert rec["buffer_equals_kept"] and rec["kept_still_there_after_sens"] and rec["rows_kept_equal_host"], rec
    rows = rec["rows"]
    assert rows["counts_equal"] and rows["status_equal"] and rows["col_equal"] and rows["len_equal"], rec
    assert rows["time_rel_max"] <= EXACT and rows["dth_ok"] and row_sum <= EXACT, rec
    assert rec["no_hit_pair"] and rec["no_hit_others_unchanged"] and rec["no_hit_no_rows"], rec
    assert join_ms > 0 and ray_ms > 0


def test_nine_lanes(ctx, envelope):
    """A request whose legs fill the device with 9-lane groups (several launches, points kept) equals
    the small request tile by tile."""
    c = _case("mixed_41x57_sg1")
    _upload(ctx, c)
    sa, sb, a_xy, b_xy = S.request(c)
    w_iz, w_ix = S.back_wall(c)
    small = ctx.skip_rays(sa, sb, a_xy, b_xy, w_iz, w_ix, check=False)
    assert ctx.get_option("ray_lanes") == 16
    n = len(sa)
    fill9 = int(ctx.get_option("n_cu")) * 4 * int(ctx.get_option("ray_waves_per_simd")) * 7
    big = (fill9 + 1) // 2 + 4
    idx = np.arange(big) % n
    got = ctx.skip_rays(sa[idx], sb[idx], a_xy[idx], b_xy[idx], w_iz, w_ix, check=False)
    lanes = ctx.get_option("ray_lanes")
    off = np.concatenate(([0], np.cumsum(small[3], dtype=np.int64)))
    tile = np.concatenate([small[5][off[k]:off[k + 1]] for k in idx])
    same = bool(np.array_equal(got[1], small[1][idx]) and _same_bits(got[0], small[0][idx]) and _same_bits(got[2], small[2][idx])
                and np.array_equal(got[3], small[3][idx]) and np.array_equal(got[4], small[4][idx])
                and _same_bits(got[5], tile))
    envelope["skip_pairs/nine_lanes"] = {"pairs": big, "lanes": lanes, "equal": same}
    assert lanes == 9 and same


def test_errors(ctx):
    """Every ALIFMM_E_ARG case returns -2 with its message, and the next valid call succeeds."""
    import _alifmm

    L = _alifmm.lib()
    fresh = _alifmm.Context(0)
    one = np.zeros(1, dtype=np.int32)
    xy1 = np.zeros((1, 2))
    with pytest.raises(_alifmm.AlifmmError, match=r"rc=-2.*no model"):
        fresh.skip_pick(one, one, one, one)
    with pytest.raises(_alifmm.AlifmmError, match=r"rc=-2.*no model"):
        fresh.skip_rays(one, one, xy1, xy1, one, one)
    fresh.close()

    c = _case("grain_41x57_sg1")
    first = 1
    _upload(ctx, c, first)
    c3 = _case("grain_41x57_sg3")
    ctx.put_field(10, 3, S.fields(c3)[0])
    sa, sb, a_xy, b_xy = S.request(c)
    sa, sb = first + sa, first + sb
    w_iz, w_ix = S.back_wall(c)
    n, nw = len(sa), len(w_iz)
    good = ctx.skip_rays(sa, sb, a_xy, b_xy, w_iz, w_ix)
    npts = len(good[5])

    def msg():
        return L.alifmm_last_error(ctx._h).decode()

    def ptr(a):
        return None if a is None else a.ctypes.data

    def pick(npairs=n, a=sa, b=sb, nnw=nw, iz=w_iz, ix=w_ix, o_pt=True, o_hit=True):
        pt, hit = np.zeros(max(n, 1)), np.zeros(max(n, 1), dtype=np.int32)
        return L.alifmm_skip_pick(ctx._h, npairs, ptr(a), ptr(b), nnw, ptr(iz), ptr(ix), ptr(pt) if o_pt else None,
                                  ptr(hit) if o_hit else None)

    def rays(npairs=n, a=sa, b=sb, axy=a_xy, bxy=b_xy, nnw=nw, iz=w_iz, ix=w_ix, o_t=True, o_len=True):
        t, ln = np.zeros(max(n, 1)), np.zeros(max(n, 1), dtype=np.int32)
        return L.alifmm_skip_rays(ctx._h, npairs, ptr(a), ptr(b), ptr(axy), ptr(bxy), nnw, ptr(iz), ptr(ix), None, None,
                                  ptr(t) if o_t else None, ptr(ln) if o_len else None, None, None, 0)

    def refused(rc, text):
        assert rc == -2 and text in msg(), (rc, text, msg())
        assert pick() == 0 and rays() == 0  # the context stays usable

    assert pick(npairs=0) == 0 and rays(npairs=0) == 0
    for call in (pick, rays):
        refused(call(npairs=-1), "npairs -1")
        refused(call(nnw=0), "nw 0")
        refused(call(a=None), "slot_a or slot_b is NULL")
        refused(call(b=None), "slot_a or slot_b is NULL")
        refused(call(iz=None), "w_iz or w_ix is NULL")
        refused(call(ix=None), "w_iz or w_ix is NULL")
        empty = sa.copy()
        empty[4] = 200
        refused(call(a=empty), "pair 4 refers to empty slot 200")
        empty[4] = -1
        refused(call(b=empty), "pair 4 refers to empty slot -1")
        mixed = sb.copy()
        mixed[6] = 10
        refused(call(b=mixed), "mixed subgrids")
        for bad_iz, bad_ix in ((c.nz, 0), (-1, 0), (0, c.nx), (0, -1)):
            iz, ix = w_iz.copy(), w_ix.copy()
            iz[5], ix[5] = bad_iz, bad_ix
            refused(call(iz=iz, ix=ix), "reflector node 5 (%d, %d) outside" % (bad_iz, bad_ix))
    refused(pick(o_pt=False), "pick_time or hit is NULL")
    refused(pick(o_hit=False), "pick_time or hit is NULL")
    refused(rays(axy=None), "a_xy or b_xy is NULL")
    refused(rays(bxy=None), "a_xy or b_xy is NULL")
    refused(rays(o_t=False), "times or ray_len is NULL")
    refused(rays(o_len=False), "times or ray_len is NULL")
    # a ray_xy buffer one point short: nothing is written, nothing is kept
    rc, pt, hit, t, ln, fl, xy = _raw_skip_rays(ctx, sa, sb, a_xy, b_xy, w_iz, w_ix, npts - 1)
    refused(rc, "ray_xy capacity %d < %d" % (npts - 1, npts))
    assert np.all(xy == -7.0) and np.all(ln == -5) and np.all(hit == -5) and np.all(t == -5.0)
    got = ctypes.c_int64(-1)
    rc = _raw_skip_rays(ctx, sa, sb, a_xy, b_xy, w_iz, w_ix, npts - 1)[0]
    assert rc == -2 and L.alifmm_take_rays(ctx._h, None, 0, ctypes.byref(got)) == 0 and got.value == 0
    # fields of one subgrid and two shapes: a slot filled under another model
    RC.set_model(ctx, RC.model("iso", 41, 61))
    ctx.put_field(11, 1, np.zeros((41, 61)))
    other = sb.copy()
    other[2] = 11
    for call in (pick, rays):
        rc = call(b=other)
        assert rc == -2 and "mixed field shapes" in msg(), msg()
    # a subgrid with more plane candidates than the ray kernel holds: the pick works, the rays are refused
    RC.set_model(ctx, RC.model("iso", 3, 3))
    ctx.put_field(12, 43, np.zeros((87, 87)))
    s12 = np.full(1, 12, dtype=np.int32)
    pt, hit = ctx.skip_pick(s12, s12, one, one)
    assert hit[0] == 0 and pt[0] == 0.0
    with pytest.raises(_alifmm.AlifmmError, match=r"rc=-2.*subgrid 43 has 261 plane candidates"):
        ctx.skip_rays(s12, s12, xy1, xy1, one, one)
    pt, hit = ctx.skip_pick(s12, s12, one, one)
    assert hit[0] == 0


def _e2e(vm):
    import Anis_TTF_rays as A

    bg, _ = S.e2e_models()
    scx = RC.DNX * np.array(S.E2E_ELEMENTS, dtype=np.float64)
    M = A.ALI_FMM(np.array(bg.veln), np.array(bg.velpn), vm, scx, np.zeros(len(scx)), group_vel=np.array(RC.TABLE),
                  phase_vel=np.array(RC.TABLE), dnx=RC.DNX)
    reflector = (np.full(bg.nx, bg.nz - 1), np.arange(bg.nx))
    times = M.find_all_skip_rays(np.array(bg.veln), np.array(bg.velpn), vm, reflector=reflector, subgrid_size=1)
    return M, times, reflector


def test_end_to_end_paths(envelope):
    """ALI_FMM.find_all_skip_rays on computed fields (iso 41 x 61, six elements on the top row, the
    back wall on the last row): no flags, every path runs from element i to element j through the hit
    node once, and the path lengths times the cells' slowness give the times."""
    bg, _ = S.e2e_models()
    M, times, reflector = _e2e(np.array(bg.vm))
    n = len(S.E2E_ELEMENTS)
    ii, jj = np.nonzero(np.triu(np.ones((n, n))))
    assert np.array_equal(np.nonzero(M.rays.ray_len), (ii, jj)) and not M.skip_flags.any()
    assert np.all(M.skip_hits[ii, jj] >= 0) and np.all(np.isfinite(M.skip_pick_times[ii, jj]))
    assert np.all(np.isnan(M.skip_pick_times[np.tril_indices(n, -1)]))
    for i, j in zip(ii, jj):
        x, z = M.ray_path(i, j)
        h = M.skip_hits[i, j]
        hx, hz = float(reflector[1][h]), float(reflector[0][h])
        assert (x[0], z[0]) == (S.E2E_ELEMENTS[i], 0.0) and (x[-1], z[-1]) == (S.E2E_ELEMENTS[j], 0.0)
        assert int(np.sum((x == hx) & (z == hz))) == 1
        assert abs(hx - 0.5 * (S.E2E_ELEMENTS[i] + S.E2E_ELEMENTS[j])) <= 1.0
    _, _, lens, pts, ctx = M._stored_rays(None)
    ctx.sens_op_build(lens, pts, subgrid=1, quantity=0)
    got = ctx.sens_op_apply(1.0 / np.array(bg.vm))  # the table's velocity is 1: a cell's slowness is 1 / vel_map
    rel = float(np.max(np.abs(got - times[ii, jj]) / times[ii, jj]))
    envelope["skip_pairs/e2e/lengths_times_slowness_vs_times_rel_max"] = rel
    assert rel <= EXACT
    # the saved store reads back
    import os
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        M.save_ray_store(os.path.join(d, "echo.npz"))
        from raystore import RayStore

        back = RayStore.load(os.path.join(d, "echo.npz"))
        assert np.array_equal(back.points, M.rays.points) and back.max_pts == 2 * 5 * (41 + 61) - 1


def test_end_to_end_tomography_step(envelope):
    """Echo times measured in the model with a vel_map block raised by 2 %: one
    tomography_step(param="vel_map") from the background strictly lowers |measured - times| after
    recomputing.  damp and smooth were chosen on the CPU chain
    (test_skip_ref.py::test_tomography_step_on_the_cpu_chain); only the decrease is asserted here."""
    bg, true = S.e2e_models()
    _, measured, _ = _e2e(np.array(true.vm))
    M, times, _ = _e2e(np.array(bg.vm))
    delta, info = M.tomography_step(measured - times, param="vel_map", damp=S.E2E_DAMP, smooth=S.E2E_SMOOTH)
    _, after, _ = _e2e(np.array(bg.vm) + delta)
    before, now = float(np.linalg.norm(measured - times)), float(np.linalg.norm(measured - after))
    envelope["skip_pairs/e2e/tomography"] = {"residual_before": before, "residual_after": now, "ratio": now / before,
                                             "iterations": info["iterations"], "reason": info["reason"]}
    assert now < before
