"""The resident sensitivity operator on the device (csrc/sens_solve.hip, host_sens.cpp alifmm_sens_op_*,
Context.sens_op_*, ALI_FMM.tomography_step) against the numpy restatement (tests/solve_ref.py, held
to numpy's lstsq by tests/test_solve_ref.py).  Run: pytest -m gpu.

The request is solve_ref.awkward_request(): synthetic rays on a 21 x 72 grid whose operator has rows
of 0 (a flagged, a one-point and an invalid ray), 1, 2, 63, 64, 65, 255, 256, 257 and 1100 entries, a
row that visits cells twice, and columns of 0, 1, 4, 5, 64, 65, 256, 257 and more than 256 (a fan of
300 rays leaving one cell) entries; the counts are asserted from the device's row_ptr and a column
histogram.  Models iso, mixed and stif65 (65 stiffness rows: past the fill kernel's LDS tables),
subgrids 1 and 3.

Bars.  Products: per element |got - ref| <= N 2^-52 sum|terms|, N the row's or column's entry
count (the maps bar of test_gpu_sens.py, and as there the reference adds the contract's own terms,
val * (cs x) per entry, with np.add.at: a one-entry row leaves no room for the two roundings by which
(val cs) x of the dense matrix differs from val (cs x); the entry-by-entry sums are held to the dense
A x and Aᵀ y at 1e-9).  Solve, on the times (quantity 1) of the mixed model at
subgrid 1: at tol = 1e-8 the true gradient |Bᵀ(b - B x)| <= 2 tol |Bᵀ b| (damp = 10 |A|_F /
sqrt(nrays) in the damped case: the restatement itself reaches 4.0e-10 |Bᵀ b| there on the CPU); at
tol = 1e-10 |x - x_lstsq| / |x_lstsq| <= 8 e_ref, e_ref the restatement's own deviation (measured on
the CPU: damp 8.2e-12, rank 1.7e-13, smooth 1.6e-13; the kernels' sums replayed on the host by
tests/solve_sim.cpp: 1.7e-11, 1.7e-13, 1.4e-13); the iteration count within 1 of the restatement's
at both tolerances (the cases are conditioned so that the restatement's own count is decided by a
wide margin, solve_ref.SOLVE_CASES);
frozen cells exactly 0.  The figures go to the session's parity envelope under "solve/..." before
anything is asserted.

Measured on the MI355X when the file was written.  Products: worst error over bound 0.23 for a row,
0.15 for a column, 0.18 against the maps of ray_sens (against A x of the dense matrix a one-entry
row had reached 0.997 of its bound).  Solve, device / restatement on that machine: true
gradient at tol = 1e-8 3.97e-10 / 8.67e-10 / 2.71e-10 of |Bᵀ b| (damp / rank / smooth; bar 2e-8);
deviation from lstsq at tol = 1e-10 1.707e-11 / 8.23e-12, 1.742e-13 / 1.59e-13, 1.419e-13 / 1.63e-13
(bar 8 e_ref); iterations 7 and 8, 11 and 12, 26 and 27 on both sides.  Every bit-reproducibility
check held; the drop-in's step brought |residual| from 2.83e-7 to 6.2e-8 (veln, 28 iterations) and
4.2e-8 (vel_map, 33 iterations).
"""
import numpy as np
import pytest

import ray_cases as RC
import sens_ref as SR
import solve_ref as V

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
NCELL = V.NZ * V.NX
E_ARG = -2


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    yield c
    c.close()


_refs = {}


def _ref(mname, sg):
    """(ray_len, xy, flags, spec, reference rows) of the awkward request; computed once."""
    if (mname, sg) not in _refs:
        ray_len, xy, flags, spec = V.awkward_request(sg)
        rows = SR.rows(SR.Model(V.model(mname)), ray_len, xy, sg, RC.DNX, flags)
        _refs[(mname, sg)] = (ray_len, xy, flags, spec, rows)
    return _refs[(mname, sg)]


def _set(ctx, mname):
    RC.set_model(ctx, V.model(mname))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _ratio(err, bound):
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))


@pytest.mark.parametrize("sg", [1, 3])
@pytest.mark.parametrize("mname", ["iso", "mixed", "stif65"])
def test_apply_against_dense(ctx, envelope, mname, sg):
    """Both products of every quantity, with a column scale of zeros, negatives and values far from
    1 and without one, against the restatement; the operator's shapes asserted from the
    device's own rows."""
    ray_len, xy, flags, spec, rows = _ref(mname, sg)
    _set(ctx, mname)
    _, csr, status = ctx.ray_sens(ray_len, xy, subgrid=sg, flags=flags, maps=False, rows=True)
    V.check_awkward(csr[0], csr[1], status, spec)
    n_row, n_col = np.diff(csr[0]), np.bincount(csr[1], minlength=NCELL)
    assert np.array_equal(csr[0], rows[0]) and np.array_equal(csr[1], rows[1])
    rng = np.random.default_rng(6)
    xin, yin = rng.normal(size=NCELL), rng.normal(size=len(ray_len))
    scale = V.col_scale()
    assert np.any(scale == 0) and np.any(scale < 0) and scale.max() >= 1e3 and scale[scale != 0].min() <= 1e-3
    for q in (0, 1, 2):
        for cs in (scale, None):
            entries, st = ctx.sens_op_build(ray_len, xy, subgrid=sg, flags=flags, quantity=q, col_scale=cs)
            assert entries == rows[0][-1] == ctx.get_option("sens_op_entries") and np.array_equal(st, rows[5])
            r_ax, m_ax, r_aty, m_aty = V.products(rows, q, NCELL, cs, xin, yin)
            A = V.dense(rows, q, NCELL, cs)
            assert np.allclose(r_ax, A @ xin, rtol=1e-9, atol=1e-20) and np.allclose(r_aty, A.T @ yin, rtol=1e-9, atol=1e-20)
            ax, aty = ctx.sens_op_apply(xin), ctx.sens_op_apply(yin, transpose=True).ravel()
            e_row, b_row = np.abs(ax - r_ax), n_row * EPS * m_ax
            e_col, b_col = np.abs(aty - r_aty), n_col * EPS * m_aty
            envelope["solve/apply/%s_sg%d_q%d_%s" % (mname, sg, q, "scaled" if cs is not None else "plain")] = {
                "rows_err_over_bound_max": _ratio(e_row, b_row), "cols_err_over_bound_max": _ratio(e_col, b_col)}
            assert np.all(e_row <= b_row) and np.all(e_col <= b_col)
            assert not ax[n_row == 0].any() and not aty[n_col == 0].any()
            if cs is not None:
                assert not aty[cs.ravel() == 0].any()


@pytest.mark.parametrize("mname,sg", [("mixed", 3), ("stif65", 1)])
def test_operator_agrees_with_ray_sens(ctx, envelope, mname, sg):
    """entries = sens_entries and the status of ray_sens for the same request; Aᵀ w without a column
    scale is map q of ray_sens(weights=w) within the maps bar."""
    ray_len, xy, flags, spec, rows = _ref(mname, sg)
    _set(ctx, mname)
    w = np.random.default_rng(5).normal(size=len(ray_len))
    w[::7] = 0.0
    maps, _, status = ctx.ray_sens(ray_len, xy, subgrid=sg, flags=flags, weights=w, maps=True)
    sens_entries = ctx.get_option("sens_entries")
    _, cnt, mag = SR.maps_of(rows, V.NZ, V.NX, w)
    for q in (0, 1, 2):
        entries, st = ctx.sens_op_build(ray_len, xy, subgrid=sg, flags=flags, quantity=q)
        assert entries == sens_entries == ctx.get_option("sens_entries") and np.array_equal(st, status)
        got = ctx.sens_op_apply(w, transpose=True)
        bound = cnt * EPS * mag[q]
        err = np.abs(got - maps[q])
        envelope["solve/vs_ray_sens/%s_sg%d_q%d" % (mname, sg, q)] = _ratio(err, bound)
        assert np.all(err <= bound)


def test_kept_points(ctx):
    """Rays traced on an uploaded field with their points kept on the device: the operator built
    from the kept points (ray_xy NULL) multiplies to the bits of the one built from the same points
    passed in, and the kept points are still there for take_rays."""
    import ctypes

    import _alifmm

    L = _alifmm.lib()
    b = [x for x in RC.TRAVEL_BATCHES if x.name == "mixed_41x57_sg3"][0]
    RC.set_model(ctx, RC.model(b.model, b.nz, b.nx))
    for k in range(len(b.fields)):
        ctx.put_field(k, b.sg, RC.field_array(b, k))
    slots = np.array([r[0] for r in b.rays], dtype=np.int32)
    src = np.array([r[1] for r in b.rays], dtype=np.float64)
    rec = np.array([r[2] for r in b.rays], dtype=np.float64)
    t, lens, flags, pts = ctx.find_rays(slots, src, rec, packed=True, check=False)
    n = len(lens)
    rng = np.random.default_rng(4)
    xin, yin = rng.normal(size=b.nz * b.nx), rng.normal(size=n)
    entries, status = ctx.sens_op_build(lens, pts, subgrid=b.sg, flags=flags, quantity=1)
    host = [ctx.sens_op_apply(xin), ctx.sens_op_apply(yin, transpose=True)]
    t2, l2, f2 = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    rc = L.alifmm_find_rays(ctx._h, n, slots.ctypes.data, src.ctypes.data, rec.ctypes.data, t2.ctypes.data, l2.ctypes.data,
                            f2.ctypes.data, None, _alifmm.KEEP_RAYS)
    assert rc == 0 and np.array_equal(l2, lens)
    kept_entries, kept_status = ctx.sens_op_build(lens, None, subgrid=b.sg, flags=flags, quantity=1)
    kept = [ctx.sens_op_apply(xin), ctx.sens_op_apply(yin, transpose=True)]
    assert kept_entries == entries > 1000 and np.array_equal(kept_status, status)
    assert all(np.array_equal(_bits(a), _bits(c)) for a, c in zip(host, kept)) and host[0].any() and host[1].any()
    # a ray's element of A x with x = 1 is its time: the ordered sum of its entries, to rounding
    ones = ctx.sens_op_apply(np.ones(b.nz * b.nx))
    live = (flags & 6) == 0
    assert np.all(np.abs(ones[live] - t[live]) <= 1e-12 * t[live])
    got = ctypes.c_int64(-1)
    back = np.empty_like(pts)
    assert L.alifmm_take_rays(ctx._h, back.ctypes.data, len(back), ctypes.byref(got)) == 0 and got.value == len(pts)
    assert np.array_equal(back, pts)
    ctx.release_fields()


def test_bit_reproducibility(ctx, envelope):
    """Apply twice; build, release, rebuild; a second context; solve twice: the same bits.  The other
    rays of the request permuted: a ray's element of A x keeps its bits."""
    import _alifmm

    ray_len, xy, flags, spec, rows = _ref("mixed", 3)
    _set(ctx, "mixed")
    cs = V.col_scale()
    rng = np.random.default_rng(8)
    xin, yin = rng.normal(size=NCELL), rng.normal(size=len(ray_len))
    rhs = 1e-8 * rng.normal(size=len(ray_len))

    def everything(c):
        c.sens_op_build(ray_len, xy, subgrid=3, flags=flags, quantity=1, col_scale=cs)
        x, info = c.sens_op_solve(rhs, damp=3e-8, smooth=1e-8, max_iter=25, tol=1e-6)
        return [c.sens_op_apply(xin), c.sens_op_apply(yin, transpose=True), x], info

    first, info = everything(ctx)
    again = [ctx.sens_op_apply(xin), ctx.sens_op_apply(yin, transpose=True)]
    x2, info2 = ctx.sens_op_solve(rhs, damp=3e-8, smooth=1e-8, max_iter=25, tol=1e-6)
    ctx.sens_op_release()
    assert ctx.get_option("sens_op_entries") == 0
    rebuilt, info3 = everything(ctx)
    other = _alifmm.Context(0)
    try:
        RC.set_model(other, V.model("mixed"))
        second, info4 = everything(other)
    finally:
        other.close()
    same = {"apply_twice": all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, again)),
            "solve_twice": np.array_equal(_bits(first[2]), _bits(x2)) and info == info2,
            "rebuilt": all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, rebuilt)) and info == info3,
            "second_context": all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, second)) and info == info4}
    # the request's rays permuted
    off = np.concatenate(([0], np.cumsum(np.maximum(ray_len, 0))))
    order = np.random.default_rng(9).permutation(len(ray_len))
    pxy = np.concatenate([xy[off[k]:off[k + 1]] for k in order])
    ctx.sens_op_build(ray_len[order], pxy, subgrid=3, flags=flags[order], quantity=1, col_scale=cs)
    permuted = ctx.sens_op_apply(xin)
    same["rows_permuted"] = np.array_equal(_bits(permuted), _bits(first[0][order]))
    envelope["solve/bit_reproducible"] = {k: bool(v) for k, v in same.items()}
    assert info["iterations"] >= 5 and np.any(first[2] != 0)
    assert all(same.values()), same


_solve_refs = {}


def _solve_ref(case):
    """The restatement's answers for a solve case: computed once, shared, left unchanged."""
    if case not in _solve_refs:
        rows, spec = _ref("mixed", 1)[4], _ref("mixed", 1)[3]
        cs, A, D, rhs, damp, smooth = V.solve_case(rows, spec, case)
        ref = V.lstsq(A, D, rhs, damp, smooth)
        x10, i10 = V.cgls(A, D, rhs, damp, smooth, 1000, 1e-10)
        x8, i8 = V.cgls(A, D, rhs, damp, smooth, 1000, 1e-8)
        _solve_refs[case] = (cs, A, D, rhs, damp, smooth, ref, V.deviation(x10, ref), i10, i8)
    return _solve_refs[case]


@pytest.mark.parametrize("case", list(V.SOLVE_CASES))
def test_solve(ctx, envelope, case):
    """damp > 0 with the wide column scale; damp = smooth = 0 on the full-column-rank case; smooth > 0
    with damp = 0 on a block of free cells.  Measured on the MI355X when written: see the module's
    docstring for the restatement's figures; the device's are in the parity envelope."""
    ray_len, xy, flags, spec, rows = _ref("mixed", 1)
    cs, A, D, rhs, damp, smooth, ref, e_ref, i10, i8 = _solve_ref(case)
    _set(ctx, "mixed")
    ctx.sens_op_build(ray_len, xy, subgrid=1, flags=flags, quantity=1, col_scale=cs)
    x8, info8 = ctx.sens_op_solve(rhs, damp=damp, smooth=smooth, max_iter=1000, tol=1e-8)
    g, g0 = V.true_gradient(A, D, rhs, damp, smooth, x8.ravel())
    x10, info10 = ctx.sens_op_solve(rhs, damp=damp, smooth=smooth, max_iter=1000, tol=1e-10)
    e_gpu = V.deviation(x10.ravel(), ref)
    envelope["solve/%s" % case] = {"true_gradient_over_BTb_tol1e-8": g / g0, "e_gpu_tol1e-10": e_gpu, "e_ref_tol1e-10": e_ref,
                                   "iterations_gpu": [info8["iterations"], info10["iterations"]],
                                   "iterations_ref": [i8["iterations"], i10["iterations"]],
                                   "solve_kernel_ms": ctx.get_option("solve_kernel_ms")}
    print("solve/%s" % case, envelope["solve/%s" % case])
    assert info8["reason"] == "tol" and info10["reason"] == "tol"
    assert g <= 2 * 1e-8 * g0, (g, g0)                                           # 4a
    assert e_gpu <= 8 * e_ref, (e_gpu, e_ref)                                    # 4b
    assert abs(info8["iterations"] - i8["iterations"]) <= 1                      # 4c
    assert abs(info10["iterations"] - i10["iterations"]) <= 1
    assert not x8[cs == 0].any() and not x10[cs == 0].any() and np.any(cs == 0)  # 4d
    assert ctx.get_option("solve_iters") == info10["iterations"] and info10["entries"] == rows[0][-1]
    for got, want in ((info10["rhs_norm"], np.linalg.norm(rhs)), (info10["grad0"], i10["grad0"]),
                      (info10["res_norm"], i10["res_norm"])):
        assert abs(got - want) <= 1e-9 * want, (got, want)
    assert info10["grad"] <= 1e-10 * info10["grad0"]


def test_solve_stops(ctx):
    """rhs = 0: breakdown (reason 2) and x = 0; max_iter = 1: one iteration, the restatement's x; an
    operator of zeros (dth on the isotropic model) with a non-zero rhs: breakdown."""
    ray_len, xy, flags, spec, rows = _ref("mixed", 1)
    cs, A, D, rhs, damp, smooth = _solve_ref("damp")[:6]
    _set(ctx, "mixed")
    ctx.sens_op_build(ray_len, xy, subgrid=1, flags=flags, quantity=1, col_scale=cs)
    x, info = ctx.sens_op_solve(np.zeros(len(ray_len)), damp=damp, smooth=damp, max_iter=10, tol=1e-8)
    assert info["reason"] == "breakdown" and info["iterations"] == 0 and not x.any()
    assert info["grad0"] == 0 and info["rhs_norm"] == 0 and info["res_norm"] == 0
    x, info = ctx.sens_op_solve(rhs, damp=damp, smooth=damp, max_iter=1, tol=1e-8)
    xr, want = V.cgls(A, D, rhs, damp, damp, 1, 1e-8)
    assert info["reason"] == "max_iter" and info["iterations"] == 1
    assert np.allclose(x.ravel(), xr, rtol=1e-11, atol=0) and x.any()
    _set(ctx, "iso")
    ctx.sens_op_build(ray_len, xy, subgrid=1, flags=flags, quantity=2)
    x, info = ctx.sens_op_solve(rhs, damp=damp, smooth=0.0, max_iter=10, tol=1e-8)
    assert info["reason"] == "breakdown" and info["iterations"] == 0 and not x.any() and info["rhs_norm"] > 0


def test_errors(ctx):
    """Every ALIFMM_E_ARG case with its message, each followed by a successful call on the same
    context."""
    import _alifmm

    L = _alifmm.lib()
    ray_len, xy, flags, spec, rows = _ref("mixed", 1)
    xy = np.ascontiguousarray(xy)
    n = len(ray_len)
    cell, ray = np.ones(NCELL), np.ones(n)
    out_c, out_r, info = np.zeros(NCELL), np.zeros(n), np.zeros(8)

    def ptr(a):
        return None if a is None else a.ctypes.data

    def build(c, sg=1, nrays=n, lens=ray_len, pts=xy, q=1, cs=None):
        rc = L.alifmm_sens_op_build(c._h, sg, nrays, ptr(lens), ptr(flags), ptr(pts), q, ptr(cs), None, None)
        return rc, L.alifmm_last_error(c._h).decode()

    def apply(c, tr=0, vin=cell, vout=out_r):
        rc = L.alifmm_sens_op_apply(c._h, tr, ptr(vin), ptr(vout))
        return rc, L.alifmm_last_error(c._h).decode()

    def solve(c, rhs=ray, damp=1e-7, smooth=0.0, max_iter=3, tol=1e-6, x=out_c):
        rc = L.alifmm_sens_op_solve(c._h, ptr(rhs), damp, smooth, max_iter, tol, ptr(x), ptr(info))
        return rc, L.alifmm_last_error(c._h).decode()

    fresh = _alifmm.Context(0)
    try:
        for call in (build, apply, solve):
            rc, msg = call(fresh)
            assert rc == E_ARG and "no model" in msg, (rc, msg)
        RC.set_model(fresh, V.model("mixed"))
        for call in (apply, solve):  # a model, never an operator
            rc, msg = call(fresh)
            assert rc == E_ARG and "no resident operator" in msg, (rc, msg)
        assert build(fresh)[0] == 0 and apply(fresh)[0] == 0
    finally:
        fresh.close()
    _set(ctx, "mixed")
    nan_cs, inf_cs = np.ones(NCELL), np.ones(NCELL)
    nan_cs[17], inf_cs[NCELL - 1] = np.nan, np.inf
    bad_builds = [(dict(sg=0), "subgrid"), (dict(nrays=-1), "nrays"), (dict(lens=None), "ray_len"),
                  (dict(pts=None), "are kept"), (dict(q=-1), "quantity"), (dict(q=3), "quantity"),
                  (dict(cs=nan_cs), "col_scale"), (dict(cs=inf_cs), "col_scale")]
    for kw, word in bad_builds:
        rc, msg = build(ctx, **kw)
        assert rc == E_ARG and word in msg, (kw, rc, msg)
        assert build(ctx)[0] == 0 and apply(ctx)[0] == 0
    for kw, word in [(dict(vin=None), "in is NULL"), (dict(vout=None), "out is NULL")]:
        rc, msg = apply(ctx, **kw)
        assert rc == E_ARG and word in msg, (kw, rc, msg)
        assert apply(ctx, 1, ray, out_c)[0] == 0
    nan_rhs, inf_rhs = ray.copy(), ray.copy()
    nan_rhs[3], inf_rhs[n - 1] = np.nan, -np.inf
    bad_solves = [(dict(rhs=None), "rhs is NULL"), (dict(x=None), "x is NULL"), (dict(rhs=nan_rhs), "rhs["),
                  (dict(rhs=inf_rhs), "rhs["), (dict(damp=-1.0), "damp"), (dict(damp=np.nan), "damp"),
                  (dict(damp=np.inf), "damp"), (dict(smooth=-1e-9), "smooth"), (dict(smooth=np.nan), "smooth"),
                  (dict(smooth=np.inf), "smooth"), (dict(max_iter=0), "max_iter"), (dict(tol=-1e-3), "tol"),
                  (dict(tol=np.nan), "tol"), (dict(tol=np.inf), "tol")]
    for kw, word in bad_solves:
        rc, msg = solve(ctx, **kw)
        assert rc == E_ARG and word in msg, (kw, rc, msg)
        rc, msg = solve(ctx)
        assert rc == 0 and info[0] >= 1, (rc, msg)
    # released: apply and solve refuse, a build brings them back
    assert L.alifmm_sens_op_release(ctx._h) == 0
    for call in (apply, solve):
        rc, msg = call(ctx)
        assert rc == E_ARG and "no resident operator" in msg, (rc, msg)
    assert build(ctx)[0] == 0 and apply(ctx)[0] == 0 and solve(ctx)[0] == 0


def test_operator_dropped_after_set_model(ctx):
    """alifmm_set_model frees the operator: apply and solve return ALIFMM_E_ARG until the next build."""
    import _alifmm

    ray_len, xy, flags, spec, rows = _ref("mixed", 1)
    _set(ctx, "mixed")
    ctx.sens_op_build(ray_len, xy, subgrid=1, flags=flags, quantity=1)
    assert ctx.get_option("sens_op_entries") == rows[0][-1]
    before = ctx.sens_op_apply(np.ones(NCELL))
    _set(ctx, "iso")
    assert ctx.get_option("sens_op_entries") == 0
    with pytest.raises(_alifmm.AlifmmError, match="no resident operator"):
        ctx.sens_op_apply(np.ones(NCELL))
    with pytest.raises(_alifmm.AlifmmError, match="no resident operator"):
        ctx.sens_op_solve(np.ones(len(ray_len)), damp=1e-7)
    _set(ctx, "mixed")
    with pytest.raises(_alifmm.AlifmmError, match="no resident operator"):
        ctx.sens_op_apply(np.ones(NCELL))
    ctx.sens_op_build(ray_len, xy, subgrid=1, flags=flags, quantity=1)
    assert np.array_equal(_bits(ctx.sens_op_apply(np.ones(NCELL))), _bits(before))


def test_dropin_tomography_step(envelope):
    """ALI_FMM.tomography_step on a 41 x 57 weld-like grain model, 6 transducers, rays at subgrid 3:
    the step equals the Context calls bit for bit for veln and vel_map, and A delta brings |residual|
    down."""
    import Anis_TTF_rays as A

    m = RC.model("grain", 41, 57)
    veln, velpn, vm, sd = (np.array(a) for a in (m.veln, m.velpn, m.vm, m.sd))
    scx = RC.DNX * np.array([5.0, 20.0, 36.0, 51.0, 12.0, 44.0])
    scz = RC.DNX * np.array([0.0, 40.0, 40.0, 0.0, 0.0, 40.0])
    M = A.ALI_FMM(veln, velpn, vm, scx, scz, stif_den=sd, dnx=RC.DNX)
    times = M.find_all_TTF_rays(veln, velpn, vm, subgrid_size=3, stif_den=sd)
    store = M.rays
    ii, jj = np.nonzero(store.ray_len)
    lens = store.ray_len[ii, jj]
    pts = np.concatenate([np.stack(store.path(i, j), axis=1) for i, j in zip(ii, jj)])
    res = 0.01 * times * np.random.default_rng(12).normal(size=times.shape)
    mask = np.ones((41, 57))
    mask[:, :3] = 0
    ctx = M._ctx(0)
    for param, q, cs in (("veln", 2, mask), ("vel_map", 1, -mask / vm)):
        unit = 1e-9 if param == "veln" else 1e-7
        delta, info = M.tomography_step(res, param=param, damp=unit, smooth=unit, max_iter=40, tol=1e-6, mask=mask)
        ctx.sens_op_build(lens, pts, subgrid=1, quantity=q, col_scale=cs)
        want, winfo = ctx.sens_op_solve(res[ii, jj], damp=unit, smooth=unit, max_iter=40, tol=1e-6)
        assert delta.shape == (41, 57) and np.array_equal(_bits(delta), _bits(want)) and info == winfo
        assert info["iterations"] >= 1 and not delta[:, :3].any() and delta.any()
        after = np.linalg.norm(res[ii, jj] - ctx.sens_op_apply(delta))
        envelope["solve/dropin/%s" % param] = {"residual_before": float(np.linalg.norm(res[ii, jj])), "residual_after": float(after),
                                               "iterations": info["iterations"], "reason": info["reason"]}
        assert after < np.linalg.norm(res[ii, jj]) and abs(after - info["res_norm"]) <= 1e-6 * info["res_norm"]
    with pytest.raises(ValueError):
        M.tomography_step(res, param="density")
