"""GPU tests of sparsity-regularised imaging over resident fields (include/alifmm.h
alifmm_tfm_sparse; csrc/tfm_sparse.hip around csrc/tfm_model.hip, csrc/tfm.hip in float64 and
csrc/trace_fir.hip) against the numpy restatement tests/tfm_sparse_ref.py.  The fields are uploaded
with put_field on the isotropic 37 x 70 model, as in test_gpu_tfm_lsq.py; the cases are
tfm_lsq_ref.CASES with five scatterers of modulus 1 to 3 and 0.01 noise, the pulses those of
test_gpu_tfm_lsq_pulse.py.

Bars.  Optimality is path-independent: with g = Bᵀ(B x - d) + R(x) from the dense matrices, the
2-norm over pixels of the distance from -g to lam ∂|x_p| is at most 2 tol G0 when L is at least the
true Lipschitz constant (-g(y) - L (x⁺ - y) lies in lam ∂|x⁺|, the gradient of f is L-Lipschitz, so
the distance is at most 2 L |x⁺ - y| = 2 Gk), and at most (1 + L_true / L_final) tol G0 when L was
found by backtracking; to either comes the rounding of the dense products themselves
(tfm_sparse_ref.kkt_rounding, a few 1e-4 of tol G0 here).  Iterates after 10 iterations agree with
fista() to 1e-11 of the iterate's norm, the iterate bar of test_gpu_tfm_lsq.py; the shrink is
continuous, so values are compared, never supports.  lam = 0 lands within 8 e_ref of numpy's lstsq,
e_ref the restatement's own deviation (the rule of test_gpu_tfm_lsq.py's _check_solve).  A sums
with atomics: no test asserts bit equality between two solves.

The restatement's figures at lam = 0.1 lam_max, tol 1e-8 (tests/test_tfm_sparse_ref.py): at most 29,
27, 46 and 77 accepted iterations on e7, e7s3, e2 and e1; its power estimate reaches 0.964 to 1.000
of the true constant in 20 rounds.  The measured figures go to the session's envelope under
tfm_sparse/... ."""
import math

import numpy as np
import pytest

import tfm_lsq_ref as L
import tfm_ref as R
import tfm_sparse_ref as S
import workloads as W

pytestmark = pytest.mark.gpu

TOL = 1e-8


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    c.set_model(np.zeros((R.NZ, R.NX)), np.ones((R.NZ, R.NX), dtype=np.int64), np.full((R.NZ, R.NX), R.SPEED), None,
                W.default_table(), W.default_table(), R.DNX)
    yield c
    c.close()


def _put(ctx, T):
    for k, f in enumerate(T):
        ctx.put_field(k, 1, f)
    return list(range(len(T)))


def _solve(ctx, Sy, rhs, **kw):
    c = Sy.c
    sl = _put(ctx, c["T"])
    return ctx.tfm_sparse(sl, sl, S.data_of(Sy, rhs), R.FS, t0=R.T0, window=c["window"], step=c["step"], pulse=Sy.h,
                          pulse_origin=Sy.origin, **kw)


def _optimality(Sy, rhs, damp, smooth, info, x):
    """(distance, rounding) of the image x from optimal, both in units of tol G0."""
    v = L.columns(x)
    unit = TOL * info["grad0"]
    return (S.kkt_distance(Sy, rhs, damp, smooth, info["lam"], v) / unit, S.kkt_rounding(Sy, rhs, damp, smooth, v) / unit)


# ---- 1. optimality ----

OPTIMAL = [(name, None, nc, damp_on, False) for name in ("e7", "e7s3") for nc in (1, 2) for damp_on in (False, True)]
OPTIMAL += [("e7s3", None, 2, True, True)] + [("e7", pk, None, True, False) for pk in S.PULSES]


@pytest.mark.parametrize("name,pk,ncomp,damp_on,smooth_on", OPTIMAL)
def test_optimality(ctx, envelope, name, pk, ncomp, damp_on, smooth_on):
    Sy, rhs, damp, smooth, xt = S.problem(name, pk, ncomp, damp_on, smooth_on)
    x, info = _solve(ctx, Sy, rhs, damp=damp, smooth=smooth, lam_rel=0.1, lipschitz=Sy.lipschitz(damp, smooth),
                     max_iter=1000, tol=TOL)
    assert x.shape == Sy.window[2:] and x.dtype == (np.complex128 if Sy.ncomp == 2 else np.float64)
    k, rnd = _optimality(Sy, rhs, damp, smooth, info, x)
    key = "tfm_sparse/optimal_%s_%s_c%d_damp%d_smooth%d" % (name, pk, Sy.ncomp, damp_on, smooth_on)
    envelope[key] = {"kkt_over_tol_G0": k, "rounding_over_tol_G0": rnd, "iterations": info["iterations"],
                     "restarts": info["restarts"], "nnz": info["nnz"], "kernel_ms": ctx.get_option("tfm_sparse_kernel_ms")}
    print(key, envelope[key])
    assert info["reason"] == "tol" and info["backtracks"] == 0
    assert k <= 2 + rnd, (k, rnd)
    assert info["nnz"] == int((S.modulus(L.columns(x)) != 0).sum())
    assert ctx.get_option("tfm_sparse_iters") == info["iterations"] and ctx.get_option("tfm_sparse_backtracks") == 0
    assert ctx.get_option("tfm_sparse_kernel_ms") > 0 and ctx.get_option("tfm_sparse_upload_ms") > 0
    assert ctx.get_option("tfm_sparse_l0") == info["lipschitz"]


@pytest.mark.parametrize("name", ["e2", "e1"])
def test_optimality_ill_conditioned(ctx, envelope, name):
    """The iteration counts are recorded, not compared."""
    Sy, rhs, damp, smooth, xt = S.problem(name, None, 2, True)
    x, info = _solve(ctx, Sy, rhs, damp=damp, lam_rel=0.1, lipschitz=Sy.lipschitz(damp, smooth), max_iter=2000, tol=TOL)
    k, rnd = _optimality(Sy, rhs, damp, smooth, info, x)
    envelope["tfm_sparse/optimal_" + name] = {"kkt_over_tol_G0": k, "iterations": info["iterations"], "nnz": info["nnz"]}
    print("tfm_sparse/optimal_" + name, envelope["tfm_sparse/optimal_" + name])
    assert info["reason"] == "tol" and k <= 2 + rnd, (k, rnd)


# ---- 2. iterates ----

def _ten(ctx, Sy, rhs, damp, smooth, lam=-0.1, **kw):
    """|x - x_ref| / |x_ref| after 10 iterations, the library against fista()."""
    lip = Sy.lipschitz(damp, smooth)
    xr, ir = S.fista(Sy, rhs, damp, smooth, lam, 10, 0.0, lipschitz=lip)
    x, info = _solve(ctx, Sy, rhs, damp=damp, smooth=smooth, lam=lam, lipschitz=lip, max_iter=10, tol=0.0, **kw)
    assert info["iterations"] == 10 and info["reason"] == "max_iter" and ir["iterations"] == 10
    assert info["restarts"] == ir["restarts"] and info["backtracks"] == 0
    return float(np.linalg.norm(L.columns(x) - xr) / np.linalg.norm(xr)), info


@pytest.mark.parametrize("name,pk,ncomp,smooth_on", [("e7", None, 1, False), ("e7s3", None, 2, True), ("e1", None, 2, False),
                                                     ("e7", "r17_c1", None, False), ("e7", "c33_c2", None, True)])
def test_iterates(ctx, envelope, name, pk, ncomp, smooth_on):
    Sy, rhs, damp, smooth, xt = S.problem(name, pk, ncomp, True, smooth_on)
    e, info = _ten(ctx, Sy, rhs, damp, smooth)
    envelope["tfm_sparse/ten_%s_%s_c%d" % (name, pk, Sy.ncomp)] = e
    print("tfm_sparse/ten_%s_%s_c%d: |x - x_ref| / |x_ref| = %.3g" % (name, pk, Sy.ncomp, e))
    assert e <= 1e-11, e


# ---- 3., 4. backtracking and the power estimate ----

@pytest.mark.parametrize("name", list(L.CASES))
@pytest.mark.parametrize("how", ["low", "power"])
def test_lipschitz_found(ctx, envelope, name, how):
    """lipschitz = 0.05 of the true constant: L is doubled until the descent test holds.  lipschitz =
    0: 20 rounds of the power method give a lower bound of the true constant, at least half of it
    (the restatement's lowest is 0.964), and the solve goes on from there."""
    Sy, rhs, damp, smooth, xt = S.problem(name, None, 2, True)
    Lt = Sy.true_lipschitz(damp, smooth)
    x, info = _solve(ctx, Sy, rhs, damp=damp, lam_rel=0.1, lipschitz=0.05 * Lt if how == "low" else 0.0, power_iters=20,
                     max_iter=2000, tol=TOL)
    l0 = ctx.get_option("tfm_sparse_l0")
    k, rnd = _optimality(Sy, rhs, damp, smooth, info, x)
    key = "tfm_sparse/%s_%s" % (how, name)
    envelope[key] = {"l0_over_true": l0 / Lt, "final_over_true": info["lipschitz"] / Lt, "backtracks": info["backtracks"],
                     "iterations": info["iterations"], "kkt_over_tol_G0": k}
    print(key, envelope[key])
    assert info["reason"] == "tol" and info["lipschitz"] <= 2 * Lt
    assert ctx.get_option("tfm_sparse_backtracks") == info["backtracks"]
    if how == "low":
        assert info["backtracks"] >= 1 and l0 == 0.05 * Lt
    else:
        assert 0.5 * Lt <= l0 <= Lt * (1 + 1e-9)
    assert k <= (1 + Lt / info["lipschitz"]) + rnd, (k, rnd)


# ---- 5. edges ----

@pytest.mark.parametrize("ncomp", [1, 2])
def test_edges(ctx, envelope, ncomp):
    Sy, rhs, damp, smooth, xt = S.problem("e7", None, ncomp, True)
    lip = Sy.lipschitz(damp, smooth)
    lam_max = float(S.modulus(Sy.tmul(rhs)).max())
    # just above lam_max: exactly +0.0 everywhere after one iteration
    x, info = _solve(ctx, Sy, rhs, damp=damp, lam=lam_max * (1 + 1e-12), lipschitz=lip, max_iter=50, tol=TOL)
    parts = (x.real, x.imag) if ncomp == 2 else (x,)
    assert info["iterations"] == 1 and info["reason"] == "tol" and info["nnz"] == 0
    assert all(not p.any() and not np.signbit(p).any() for p in parts)
    assert abs(info["lam_max"] - lam_max) <= 1e-12 * lam_max
    # lam = 0: least squares
    xl = L.lstsq(Sy.B, Sy.D, rhs, damp, smooth)
    xr, ir = S.fista(Sy, rhs, damp, smooth, 0.0, 2000, 1e-10, lipschitz=lip)
    e_ref = L.deviation(xr, xl)
    x0, info0 = _solve(ctx, Sy, rhs, damp=damp, lam=0.0, lipschitz=lip, max_iter=2000, tol=1e-10)
    e_gpu = L.deviation(L.columns(x0), xl)
    envelope["tfm_sparse/lam0_c%d" % ncomp] = {"e_gpu": e_gpu, "e_ref": e_ref, "iterations": info0["iterations"],
                                              "iterations_ref": ir["iterations"]}
    print("tfm_sparse/lam0_c%d" % ncomp, envelope["tfm_sparse/lam0_c%d" % ncomp])
    assert info0["reason"] == "tol" and info0["nnz"] == Sy.npix
    assert e_gpu <= 8 * e_ref, (e_gpu, e_ref)
    # a relative lam is the same absolute lam
    kw = dict(damp=damp, lipschitz=lip, max_iter=10, tol=0.0)
    xa, ia = _solve(ctx, Sy, rhs, lam=0.3 * lam_max, **kw)
    xn, inn = _solve(ctx, Sy, rhs, lam=-0.3, **kw)
    xq, iq = _solve(ctx, Sy, rhs, lam_rel=0.3, **kw)
    n = np.linalg.norm(xa)
    assert n > 0 and np.linalg.norm(xn - xa) <= 1e-11 * n and np.linalg.norm(xq - xa) <= 1e-11 * n
    assert abs(inn["lam"] - 0.3 * lam_max) <= 1e-12 * lam_max and ia["lam"] == 0.3 * lam_max
    # the residual is computed from the returned image
    x, info, res = _solve(ctx, Sy, rhs, damp=damp, lam_rel=0.1, lipschitz=lip, max_iter=1000, tol=TOL, resid=True)
    d = S.data_of(Sy, rhs)
    assert res.shape == d.shape and res.dtype == d.dtype
    want = rhs - Sy.mul(L.columns(x))
    err = np.linalg.norm(Sy.rhs_of(res) - want)
    print("resid c%d: |r - (d - B x)| = %.3g |d|" % (ncomp, err / info["rhs_norm"]))
    assert err <= 1e-11 * info["rhs_norm"]
    assert abs(info["res_norm"] - np.linalg.norm(want)) <= 1e-11 * info["rhs_norm"]
    assert abs(info["rhs_norm"] - np.linalg.norm(rhs)) <= 1e-12 * info["rhs_norm"]


def test_zero_data_breaks_down(ctx):
    Sy, rhs, damp, smooth, xt = S.problem("e7", None, 2, True)
    x, info = _solve(ctx, Sy, np.zeros(rhs.shape), damp=damp, lam_rel=0.1, max_iter=10)
    assert info["reason"] == "breakdown" and info["iterations"] == 0 and info["grad0"] == 0 and info["nnz"] == 0
    assert not x.real.any() and not x.imag.any()


# ---- 6. long sums ----

def test_long_sums(ctx, envelope):
    """12 elements, complex, nt = 1024: a data vector of 294 912 elements, more than the 262 144
    lanes of a two-stage sum, so lanes add more than one term.  Optimality only."""
    n, nt = 12, 1024
    assert n * n * nt * 2 > 1024 * 256
    T = R.fields(R.element_x(n))
    fs = nt / 480 * R.FS
    win = L.CASES["e7"][1]
    A = L.dense_A(T, T, nt, fs, R.T0, None, win, 1)
    Sy = S.System(A, L.difference(*win[2:]), 2, False, win)
    xt = S.truth(Sy)
    rhs = A @ xt + L.NOISE * np.random.default_rng(61).standard_normal((A.shape[0], 2))
    damp = L.DAMP * Sy.smax
    sl = _put(ctx, T)
    x, info = ctx.tfm_sparse(sl, sl, L.from_columns(rhs, (n, n, nt)), fs, t0=R.T0, window=win, damp=damp, lam_rel=0.1,
                             lipschitz=Sy.lipschitz(damp, 0.0), max_iter=1000, tol=TOL)
    k, rnd = _optimality(Sy, rhs, damp, 0.0, info, x)
    envelope["tfm_sparse/long_sums"] = {"kkt_over_tol_G0": k, "rounding_over_tol_G0": rnd, "iterations": info["iterations"],
                                        "nnz": info["nnz"]}
    print("tfm_sparse/long_sums", envelope["tfm_sparse/long_sums"])
    assert info["reason"] == "tol" and k <= 2 + rnd, (k, rnd)
    assert abs(info["rhs_norm"] - np.linalg.norm(rhs)) <= 1e-12 * info["rhs_norm"]


# ---- 7. the paths of the modelling kernel inside the loop ----

def test_model_paths_in_the_loop(ctx, envelope):
    """tfm_model_slabs = 2 (what A writes is zeroed before every product) and tfm_model_rx 1 and 4,
    under the complex pulse: ten iterations against the restatement's."""
    Sy, rhs, damp, smooth, xt = S.problem("e7", "c33_c2", None, True, True)
    rx0 = ctx.get_option("tfm_model_rx")
    try:
        for opt, val in (("tfm_model_slabs", 2), ("tfm_model_rx", 1), ("tfm_model_rx", 4)):
            ctx.set_option(opt, val)
            e, info = _ten(ctx, Sy, rhs, damp, smooth)
            ctx.set_option(opt, 0 if opt == "tfm_model_slabs" else rx0)
            envelope["tfm_sparse/ten_%s%d" % (opt, val)] = e
            print("tfm_sparse/ten_%s%d: |x - x_ref| / |x_ref| = %.3g" % (opt, val, e))
            assert e <= 1e-11, (opt, val, e)
            assert opt != "tfm_model_slabs" or ctx.get_option("tfm_model_slabs_used") == 2
    finally:
        ctx.set_option("tfm_model_slabs", 0)
        ctx.set_option("tfm_model_rx", rx0)


# ---- 8. what it is for ----

def test_what_it_is_for(ctx, envelope):
    """Five scatterers seen through the 17-tap pulse.  The damped least-squares image (damp = 1e-2
    sigma_max) is non-zero in more than half the window; the sparse image at lam = 0.1 lam_max holds
    the five true pixels among at most 15 non-zero ones."""
    Sy, rhs, damp, smooth, xt = S.problem("e7", "r17_c1", None, True)
    c = Sy.c
    sl = _put(ctx, c["T"])
    kw = dict(t0=R.T0, window=c["window"], step=c["step"], pulse=Sy.h, pulse_origin=Sy.origin, max_iter=1000, tol=TOL)
    xl, il = ctx.tfm_lsq(sl, sl, S.data_of(Sy, rhs), R.FS, damp=damp, **kw)
    xs, isp = ctx.tfm_sparse(sl, sl, S.data_of(Sy, rhs), R.FS, lam_rel=0.1, **kw)
    true = set(np.nonzero(S.modulus(xt))[0])
    sup_s = set(np.nonzero(S.modulus(L.columns(xs)))[0])
    sup_l = set(np.nonzero(S.modulus(L.columns(xl)))[0])
    e = {"support_sparse": len(sup_s), "support_lsq": len(sup_l), "pixels": Sy.npix,
         "map_error_sparse": L.deviation(L.columns(xs), xt), "map_error_lsq": L.deviation(L.columns(xl), xt),
         "iterations_sparse": isp["iterations"], "iterations_lsq": il["iterations"]}
    envelope["tfm_sparse/what_it_is_for"] = e
    print("tfm_sparse/what_it_is_for", e)
    assert isp["reason"] == "tol" and il["reason"] == "tol"
    assert true <= sup_s and len(sup_s) <= 3 * len(true) and isp["nnz"] == len(sup_s)
    assert len(sup_l) > Sy.npix / 2


# ---- 9. errors ----

def test_errors(ctx):
    """Every rejected input raises with rc=-2 and a message that names tfm_sparse, leaves the outputs
    as they were and is followed by a valid call on the same context."""
    import _alifmm

    E = _alifmm.AlifmmError
    Sy, rhs, damp, smooth, xt = S.problem("e7", "c33_c2", None, True)
    c, h, origin = Sy.c, Sy.h, Sy.origin
    win = c["window"]
    sl = _put(ctx, c["T"])
    ctx.put_field(7, 3, np.zeros((109, 208)))
    d = S.data_of(Sy, rhs)
    lip = Sy.lipschitz(damp, 0.0)
    kw = dict(t0=R.T0, window=win, damp=damp, max_iter=3, lam_rel=0.1, lipschitz=lip)
    dn = d.copy()
    dn[6, 6, R.NT - 1] = complex(0.0, np.nan)
    hn = h.copy()
    hn[5] = complex(np.nan, 0.0)

    def but(**over):
        k = dict(kw)
        k.update(over)
        return k

    bad = [
        lambda: ctx.tfm_sparse([0, 999] + sl[2:], sl, d, R.FS, **kw),            # the conditions of alifmm_tfm_lsq_pulse
        lambda: ctx.tfm_sparse(sl, sl[:6] + [7], d, R.FS, **kw),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, subgrid=3, **kw),
        lambda: ctx.tfm_sparse(sl, sl, d[:, :, :1], R.FS, **kw),
        lambda: ctx.tfm_sparse(sl, sl, d, -R.FS, **kw),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, **but(t0=math.nan)),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, step=0, **kw),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, **but(window=(0, 0, R.NZ + 1, R.NX))),
        lambda: ctx.tfm_sparse(sl, sl, dn, R.FS, **kw),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, **but(damp=-1.0)),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, smooth=math.inf, **kw),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, **but(max_iter=0)),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, tol=-1e-3, **kw),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, pulse=np.ones(1025), **kw),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, pulse=h, pulse_origin=len(h), **kw),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, pulse=hn, pulse_origin=origin, **kw),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, **but(lam_rel=None, lam=math.nan)),    # lam, lipschitz, power_iters
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, **but(lam_rel=None, lam=math.inf)),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, **but(lam_rel=None, lam=-math.inf)),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, **but(lipschitz=-1.0)),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, **but(lipschitz=math.nan)),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, **but(lipschitz=math.inf)),
        lambda: ctx.tfm_sparse(sl, sl, d, R.FS, **but(lipschitz=0.0), power_iters=0),
    ]
    # what only the C-ABI can express: restart, null pointers, the taps' shape
    si = np.asarray(sl, dtype=np.int32)
    dc = L.as_samples64(d)
    taps = np.ascontiguousarray(h).view(np.float64).reshape(-1, 2)
    img = np.full(win[2:] + (2,), 123.0)
    res = np.full(dc.shape, 123.0)
    info = np.full(12, 123.0)
    p = lambda a: None if a is None else a.ctypes.data

    def raw(data=dc, ncomp=2, ntap=33, tap_comp=2, tp=taps, org=origin, lam=-0.1, lipschitz=lip, power_iters=20, restart=1,
            image=img, inf=info, max_iter=3, tol=1e-6):
        rc = _alifmm.lib().alifmm_tfm_sparse(ctx._h, 1, 7, p(si), 7, p(si), p(data), R.NT, ncomp, R.T0, R.FS, None, *win, 1,
                                             damp, 0.0, max_iter, tol, ntap, tap_comp, p(tp), org, lam, lipschitz,
                                             power_iters, restart, p(image), p(res), p(inf))
        ctx._chk(rc, "tfm_sparse")

    bad += [
        lambda: raw(restart=2),
        lambda: raw(restart=-1),
        lambda: raw(inf=None),
        lambda: raw(image=None),
        lambda: raw(data=None),
        lambda: raw(ncomp=3),
        lambda: raw(tap_comp=3),
        lambda: raw(tp=None),               # taps NULL with ntap 33
        lambda: raw(ntap=0),                # ntap 0 with taps
        lambda: raw(data=np.ascontiguousarray(dc[..., 0]), ncomp=1),  # complex taps with real data
    ]
    for k, call in enumerate(bad):
        with pytest.raises(E, match=r"rc=-2\): tfm_sparse|tfm_sparse: step"):
            call()
            pytest.fail("rejected input %d was accepted" % k)
    assert (img == 123.0).all() and (res == 123.0).all() and (info == 123.0).all()
    # the Python layer's own checks
    with pytest.raises(ValueError, match="lam"):
        ctx.tfm_sparse(sl, sl, d, R.FS, **but(lam=1.0))
    with pytest.raises(ValueError, match="lam"):
        ctx.tfm_sparse(sl, sl, d, R.FS, **but(lam_rel=None))
    with pytest.raises(ValueError, match="complex pulse"):
        ctx.tfm_sparse(sl, sl, d.real, R.FS, pulse=h, **kw)
    # the context is still usable: valid calls pass, raw (ntap 0 and taps NULL: no pulse) and through Python
    raw(max_iter=1000, tol=TOL)
    assert info[5] == 0 and (img != 123.0).any() and (res != 123.0).any()
    k = S.kkt_distance(Sy, rhs, damp, 0.0, info[7], img.reshape(-1, 2))
    assert k <= 2 * TOL * info[1] + S.kkt_rounding(Sy, rhs, damp, 0.0, img.reshape(-1, 2))
    raw(ntap=0, tp=None, tap_comp=0, org=0, max_iter=5, tol=0.0, lipschitz=0.0)
    assert info[0] == 5 and info[5] == 1
    x, inf = _solve(ctx, Sy, rhs, damp=damp, lam_rel=0.1, lipschitz=lip, max_iter=1000, tol=TOL)
    assert inf["reason"] == "tol"


# ---- 10. the drop-in ----

def test_end_to_end_through_the_dropin(envelope):
    """ALI_FMM.sparse_image on computed fields (the 61² Voronoi model and 8 elements of
    test_gpu_tfm_lsq.py's drop-in test), five scatterers seen through the 17-tap pulse: ten
    iterations equal fista() on the dense matrix of the named slots' fields and Context.tfm_sparse on
    those slots; the converged image is optimal; a relative lam is the library's own."""
    import Anis_TTF_rays as A
    import trace_fir_ref as F

    n, dnx, fs = 61, 1e-3, R.FS
    veln = W.voronoi_small(n, seed=7)
    velpn = np.zeros((n, n), dtype=np.int64)
    vm = np.ones((n, n))
    sd = W.stif_field(n, n)
    xs = np.arange(6, 56, 7)
    Mo = A.ALI_FMM(veln, velpn, vm, dnx * xs.astype(float), np.zeros(8), stif_den=sd, dnx=dnx)
    F0 = Mo.update(veln, velpn, vm, sd)
    win = (20, 15, 12, 17)
    h = F.pulse(17, 3, False)
    nt = math.ceil(2 * F0.max() * fs) + 2 + len(h)
    Sy0 = S.System(np.zeros((1, win[2] * win[3])), L.difference(*win[2:]), 1, False, win)
    x_true = S.truth(Sy0).reshape(win[2:])
    d = Mo.simulate_fmc(x_true, fs, nt, window=win, pulse=h)
    d = d + L.NOISE * np.random.default_rng(62).standard_normal(d.shape)
    c = Mo._ctx(0)
    txs, rxs = Mo._pair_slots("sparse_image", None, None, 1, None, None, None, None, "direct", "direct", None)
    T = np.stack([c.get_field(k, 1) for k in txs])
    Sy = S.System(F.dense_PA(L.dense_A(T, T, nt, fs, 0.0, None, win, 1), 64, nt, h, 0, 1), Sy0.D, 1, False, win)
    rhs = L.columns(d)
    damp = 1e-3 * Sy.smax
    lip = Sy.lipschitz(damp, 0.0)
    kw = dict(window=win, damp=damp, pulse=h, pulse_origin=0, lipschitz=lip)
    xr, ir = S.fista(Sy, rhs, damp, 0.0, -0.1, 10, 0.0, lipschitz=lip)
    x10, i10 = Mo.sparse_image(d, fs, lam_rel=0.1, max_iter=10, tol=0.0, **kw)
    xc, ic = c.tfm_sparse(txs, rxs, d, fs, lam_rel=0.1, max_iter=10, tol=0.0, **kw)
    nrm = np.linalg.norm(xr)
    e = {"ten_vs_ref": float(np.linalg.norm(L.columns(x10) - xr) / nrm),
         "ten_vs_context": float(np.linalg.norm(x10 - xc) / nrm)}
    img, info = Mo.sparse_image(d, fs, max_iter=1000, tol=TOL, **kw)  # lam_rel = 0.1 is the default
    v = L.columns(img)
    k = S.kkt_distance(Sy, rhs, damp, 0.0, info["lam"], v) / (TOL * info["grad0"])
    rnd = S.kkt_rounding(Sy, rhs, damp, 0.0, v) / (TOL * info["grad0"])
    e.update(kkt_over_tol_G0=k, iterations=info["iterations"], nnz=info["nnz"], map_error=L.deviation(img, x_true),
             true_in_support=bool(set(np.nonzero(x_true.ravel())[0]) <= set(np.nonzero(img.ravel())[0])))
    envelope["tfm_sparse/dropin"] = e
    print("tfm_sparse/dropin", e)
    assert img.shape == win[2:] and img.dtype == np.float64 and info["reason"] == "tol"
    assert e["ten_vs_ref"] <= 1e-11 and e["ten_vs_context"] <= 1e-11, e
    assert abs(info["lam"] - 0.1 * info["lam_max"]) <= 1e-15 * info["lam_max"]
    assert abs(info["lam_max"] - S.modulus(Sy.tmul(rhs)).max()) <= 1e-12 * info["lam_max"]
    assert k <= 2 + rnd, (k, rnd)
    # an absolute lam takes over from lam_rel
    xa, ia = Mo.sparse_image(d, fs, lam=0.5 * info["lam_max"], max_iter=10, tol=0.0, **kw)
    assert ia["lam"] == 0.5 * info["lam_max"] and ia["iterations"] == 10
    with pytest.raises(IndexError, match="sparse_image"):
        Mo.sparse_image(d, fs, window=win, tx=[8])
