"""GPU tests of pulse-aware least-squares imaging (include/alifmm.h alifmm_tfm_lsq_pulse: the CGLS
of alifmm_tfm_lsq on the operator B = P A, csrc/trace_fir.hip around csrc/tfm_model.hip and
csrc/tfm.hip) against the numpy restatement: tfm_lsq_ref.cgls() on the dense matrix
trace_fir_ref.dense_PA().  The fields are uploaded with put_field on the isotropic 37 x 70 model, as
in test_gpu_tfm_lsq.py.

Bars.  They are test_gpu_tfm_lsq.py's, not new numbers: the FIR has a fixed order (bit-exact
against its restatement, test_gpu_trace_fir.py), so it adds no source of error; A sums with atomics
as before.  A solve at tol 1e-8: the true gradient of the stacked dense system is at most
2 tol |Bᵀ b|.  At tol 1e-10: within 8 e_ref of numpy's lstsq (e_ref the restatement's own
deviation), iterations within 1 of the restatement's on the well-conditioned cases (recorded, not
compared, on the ill-conditioned ones: long CGLS runs lose orthogonality and their counts differ
between any two summation orders), the norms within 1e-9, the final gradient under the stop rule.
Iterates after a fixed number of iterations: 1e-11 relative to the iterate's norm.  The measured
figures go to the session's envelope under tfm_lsq_pulse/... .

Unknowns and data.  With a real pulse the operator acts component-wise: B is (rows, pixels) and a
complex problem has two columns, as in tfm_lsq_ref.  A complex pulse mixes the components: B is
then the real matrix on interleaved unknowns and interleaved data, and the vectors are flat."""
import math

import numpy as np
import pytest

import tfm_lsq_ref as L
import tfm_ref as R
import trace_fir_ref as F
import workloads as W

pytestmark = pytest.mark.gpu

# name -> (pulse, ncomp): the pulses of the issue, origin = ntap // 2
PULSES = {"r17_c1": (F.pulse(17, 3, False), 1), "r17_c2": (F.pulse(17, 3, False), 2), "c33_c2": (F.pulse(33, 5, True), 2)}


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


# ---- the reference systems (computed once, never modified) ----

_sys, _refs = {}, {}


def _system(name, pk):
    """dict(c, h, origin, ncomp, flat, B, D, smax) of case `name` under pulse `pk`."""
    if (name, pk) not in _sys:
        c = L.case(name)
        h, ncomp = PULSES[pk]
        origin = len(h) // 2
        flat = np.iscomplexobj(h)
        B = F.dense_PA(c["A"], c["n"] ** 2, R.NT, h, origin, 2 if flat else 1)
        D = F.dense_D(c["D"], 2) if flat else c["D"]
        smax = float(np.sqrt(np.linalg.eigvalsh(B.T @ B)[-1]))  # (the largest one: no loss in the squaring)
        B.setflags(write=False)
        _sys[name, pk] = dict(c=c, h=h, origin=origin, ncomp=ncomp, flat=flat, B=B, D=D, smax=smax)
    return _sys[name, pk]


def _vec(s, img):
    """An image of the library -> the unknown vector of the system."""
    v = L.columns(img)
    return v.ravel() if s["flat"] else v


def _data(s, rhs):
    """A right-hand side of the system -> the data array (n, n, nt) the library takes."""
    return L.data_of(s["c"], rhs.reshape(-1, s["ncomp"]))


def _rhs(s, data):
    v = L.columns(data)
    return v.ravel() if s["flat"] else v


def _problem(name, pk, smooth_on):
    """(system, rhs, damp, smooth): rhs = B x_true + 0.01 noise, damp = 1e-2 sigma_max(B)."""
    s = _system(name, pk)
    key = (name, pk, "rhs")
    if key not in _sys:
        rng = np.random.default_rng(90 + len(pk) + 7 * s["ncomp"])
        shape = (lambda n: (n * 2,)) if s["flat"] else (lambda n: (n, s["ncomp"]))
        rhs = s["B"] @ rng.standard_normal(shape(s["c"]["A"].shape[1])) + L.NOISE * rng.standard_normal(shape(s["c"]["A"].shape[0]))
        rhs.setflags(write=False)
        _sys[key] = rhs
    damp = L.DAMP * s["smax"]
    return s, _sys[key], damp, damp if smooth_on else 0.0


def _solve_ref(name, pk, smooth_on):
    key = (name, pk, smooth_on)
    if key not in _refs:
        s, rhs, damp, smooth = _problem(name, pk, smooth_on)
        xl = L.lstsq(s["B"], s["D"], rhs, damp, smooth)
        x10, i10, _ = L.cgls(s["B"], s["D"], rhs, damp, smooth, 1000, 1e-10)
        x8, i8, _ = L.cgls(s["B"], s["D"], rhs, damp, smooth, 1000, 1e-8)
        assert i8["reason"] == "tol" and i10["reason"] == "tol"
        _refs[key] = (s, rhs, damp, smooth, xl, L.deviation(x10, xl), i10, i8)
    return _refs[key]


def _solve(ctx, s, rhs, **kw):
    c = s["c"]
    sl = _put(ctx, c["T"])
    return ctx.tfm_lsq(sl, sl, _data(s, rhs), R.FS, t0=R.T0, window=c["window"], step=c["step"], pulse=s["h"],
                       pulse_origin=s["origin"], **kw)


def _check_solve(ctx, envelope, name, pk, smooth_on, compare_iterations):
    s, rhs, damp, smooth, xl, e_ref, i10, i8 = _solve_ref(name, pk, smooth_on)
    x8, info8 = _solve(ctx, s, rhs, damp=damp, smooth=smooth, max_iter=1000, tol=1e-8)
    assert x8.shape == s["c"]["window"][2:] and x8.dtype == (np.complex128 if s["ncomp"] == 2 else np.float64)
    g, g0 = L.true_gradient(s["B"], s["D"], rhs, damp, smooth, _vec(s, x8))
    x10, info10 = _solve(ctx, s, rhs, damp=damp, smooth=smooth, max_iter=1000, tol=1e-10)
    e_gpu = L.deviation(_vec(s, x10), xl)
    key = "tfm_lsq_pulse/solve_%s_%s%s" % (name, pk, "_smooth" if smooth_on else "")
    envelope[key] = {"true_gradient_over_BTb_tol1e-8": g / g0, "e_gpu_tol1e-10": e_gpu, "e_ref_tol1e-10": e_ref,
                     "iterations_gpu": [info8["iterations"], info10["iterations"]],
                     "iterations_ref": [i8["iterations"], i10["iterations"]],
                     "tfm_lsq_kernel_ms": ctx.get_option("tfm_lsq_kernel_ms")}
    print(key, envelope[key])
    assert info8["reason"] == "tol" and info10["reason"] == "tol"
    assert g <= 2 * 1e-8 * g0, (g, g0)
    assert e_gpu <= 8 * e_ref, (e_gpu, e_ref)
    if not compare_iterations:
        return
    assert abs(info10["iterations"] - i10["iterations"]) <= 1
    assert ctx.get_option("tfm_lsq_iters") == info10["iterations"]
    for got, want in ((info10["rhs_norm"], i10["rhs_norm"]), (info10["grad0"], i10["grad0"]),
                      (info10["res_norm"], i10["res_norm"])):
        assert abs(got - want) <= 1e-9 * want, (got, want)
    assert info10["grad"] <= 1e-10 * info10["grad0"]


# ---- 1., 2. solves ----

@pytest.mark.parametrize("pk", list(PULSES))
@pytest.mark.parametrize("name", ["e7", "e7s3"])
def test_solve(ctx, envelope, name, pk):
    _check_solve(ctx, envelope, name, pk, False, True)


def test_solve_smooth(ctx, envelope):
    """smooth = damp on the 10 x 20 window at step 3 under the complex pulse."""
    _check_solve(ctx, envelope, "e7s3", "c33_c2", True, True)


@pytest.mark.parametrize("pk", list(PULSES))
@pytest.mark.parametrize("name", ["e2", "e1"])
def test_solve_ill_conditioned(ctx, envelope, name, pk):
    _check_solve(ctx, envelope, name, pk, False, False)


def test_solve_ill_conditioned_smooth(ctx, envelope):
    _check_solve(ctx, envelope, "e1", "r17_c1", True, False)


# ---- 3. the paths of the modelling kernel inside the loop ----

def test_model_paths_in_the_loop(ctx, envelope):
    """Three iterations against the restatement's three under the complex pulse: tfm_model_slabs 1
    and 4 (w, not q, is what is zeroed every iteration) and tfm_model_tile 64."""
    s, rhs, damp, _ = _problem("e7", "c33_c2", True)
    xr, ir, _ = L.cgls(s["B"], s["D"], rhs, damp, damp, 3, 0.0)

    def three(name):
        x, info = _solve(ctx, s, rhs, damp=damp, smooth=damp, max_iter=3, tol=0.0)
        e = np.linalg.norm(_vec(s, x) - xr) / np.linalg.norm(xr)
        envelope["tfm_lsq_pulse/three_" + name] = e
        print("tfm_lsq_pulse/three_%s: |x - x_ref| / |x_ref| = %.3g" % (name, e))
        assert info["iterations"] == 3 and info["reason"] == "max_iter"
        assert e <= 1e-11, (name, e)

    try:
        for slabs in (1, 4):
            ctx.set_option("tfm_model_slabs", slabs)
            three("slabs%d" % slabs)
            assert ctx.get_option("tfm_model_slabs_used") == slabs
        ctx.set_option("tfm_model_slabs", 0)
        ctx.set_option("tfm_model_tile", 64)
        three("tile64")
        assert ctx.get_option("tfm_model_tile_used") == 64
    finally:
        ctx.set_option("tfm_model_slabs", 0)
        ctx.set_option("tfm_model_tile", 0)


# ---- 4. the residual ----

@pytest.mark.parametrize("pk", list(PULSES))
def test_resid(ctx, pk):
    s, rhs, damp, _ = _problem("e7s3", pk, False)
    x, info, res = _solve(ctx, s, rhs, damp=damp, max_iter=1000, tol=1e-8, resid=True)
    d = _data(s, rhs)
    assert res.shape == d.shape and res.dtype == d.dtype
    want = rhs - s["B"] @ _vec(s, x)
    err = np.abs(_rhs(s, res) - want).max()
    print("resid %s: max |r - (b - B x)| = %.3g, |b| = %.3g" % (pk, err, info["rhs_norm"]))
    assert err <= 1e-12 * info["rhs_norm"]
    assert abs(info["res_norm"] - np.linalg.norm(L.columns(res))) <= 1e-12 * info["res_norm"]
    assert info["res_norm"] < info["rhs_norm"]


# ---- 5., 6. the neutral pulse and the dispatch ----

def _raw_plain(ctx, c, d, damp, smooth, max_iter, tol):
    """alifmm_tfm_lsq itself, as test_gpu_tfm_lsq.py calls it."""
    import _alifmm

    sl = np.asarray(_put(ctx, c["T"]), dtype=np.int32)
    dc = L.as_samples64(d)
    nc = dc.shape[-1]
    img = np.zeros(c["window"][2:] + (nc,))
    info = np.zeros(8)
    rc = _alifmm.lib().alifmm_tfm_lsq(ctx._h, 1, len(sl), sl.ctypes.data, len(sl), sl.ctypes.data, dc.ctypes.data, R.NT, nc,
                                      R.T0, R.FS, None, *c["window"], c["step"], damp, smooth, max_iter, tol,
                                      img.ctypes.data, None, info.ctypes.data)
    ctx._chk(rc, "tfm_lsq")
    return L.columns(img.view(np.complex128)[..., 0] if nc == 2 else img[..., 0]), info


@pytest.mark.parametrize("ncomp", [1, 2])
def test_neutral_pulse_and_dispatch(ctx, envelope, ncomp):
    """pulse = [1.0] at origin 0 is the identity: three iterations agree with the pulse-less solve
    (the operator is identical; the modelling sums are atomic, so no bit equality).  And pulse=None
    is the pulse-less entry point itself, with what it returned before."""
    c, rhs, damp, _ = L.problem("e7", ncomp)
    d = L.data_of(c, rhs)
    sl = _put(ctx, c["T"])
    kw = dict(t0=R.T0, window=c["window"], step=c["step"], damp=damp, smooth=damp, max_iter=3, tol=0.0)
    xr = L.cgls(c["A"], c["D"], rhs, damp, damp, 3, 0.0)[0]
    plain, info_p = _raw_plain(ctx, c, d, damp, damp, 3, 0.0)
    none, info_n = ctx.tfm_lsq(sl, sl, d, R.FS, pulse=None, **kw)
    default, _ = ctx.tfm_lsq(sl, sl, d, R.FS, **kw)
    one, info_1 = ctx.tfm_lsq(sl, sl, d, R.FS, pulse=[1.0], pulse_origin=0, **kw)
    n = np.linalg.norm(xr)
    e = {"plain": np.linalg.norm(plain - xr) / n, "none": np.linalg.norm(L.columns(none) - plain) / n,
         "default": np.linalg.norm(L.columns(default) - plain) / n, "one": np.linalg.norm(L.columns(one) - plain) / n}
    envelope["tfm_lsq_pulse/neutral_c%d" % ncomp] = e
    print("tfm_lsq_pulse/neutral_c%d" % ncomp, e)
    assert all(v <= 1e-11 for v in e.values()), e
    assert info_n["iterations"] == 3 and info_1["iterations"] == 3 and info_p[0] == 3
    for k, key in ((1, "grad0"), (3, "rhs_norm"), (4, "res_norm")):
        assert abs(info_n[key] - info_p[k]) <= 1e-11 * info_p[k] and abs(info_1[key] - info_p[k]) <= 1e-11 * info_p[k]


# ---- 7. the point of the feature ----

@pytest.mark.parametrize("pk", list(PULSES))
def test_the_pulse_has_to_be_in_the_operator(ctx, envelope, pk):
    """Three scatterers seen through the pulse: the pulse-aware solve recovers them, the pulse-less
    solve on the same data cannot even fit them."""
    s = _system("e7", pk)
    c = s["c"]
    x_true = np.zeros((c["A"].shape[1], s["ncomp"]))
    x_true[20, 0], x_true[58, 0], x_true[100, 0] = 1.0, -0.7, 0.5
    if s["ncomp"] == 2:
        x_true[58, 1] = 0.4
    xt = x_true.ravel() if s["flat"] else x_true
    rhs = s["B"] @ xt
    damp = 1e-3 * s["smax"]
    x, info = _solve(ctx, s, rhs, damp=damp, max_iter=1000, tol=1e-8)
    sl = _put(ctx, c["T"])
    x0, info0 = ctx.tfm_lsq(sl, sl, _data(s, rhs), R.FS, t0=R.T0, window=c["window"], step=c["step"], damp=damp,
                            max_iter=1000, tol=1e-8)
    e = {"res_over_rhs": info["res_norm"] / info["rhs_norm"], "x_error": L.deviation(_vec(s, x), xt),
         "iterations": info["iterations"], "pulse_less_res_over_rhs": info0["res_norm"] / info0["rhs_norm"],
         "pulse_less_x_error": L.deviation(_vec(s, x0), xt), "pulse_less_iterations": info0["iterations"]}
    envelope["tfm_lsq_pulse/point_" + pk] = e
    print("tfm_lsq_pulse/point_" + pk, e)
    assert info["reason"] == "tol" and info0["reason"] == "tol"
    assert e["res_over_rhs"] < 1e-4 and e["x_error"] < 1e-3
    assert e["pulse_less_res_over_rhs"] > 0.5


# ---- 8. errors of the new entry ----

def test_errors(ctx):
    """The tap conditions raise with rc=-2 (the Python layer's own with ValueError), leave the
    outputs as they were and are followed by a valid call."""
    import _alifmm

    E = _alifmm.AlifmmError
    s, rhs, damp, smooth, xl, e_ref, i10, i8 = _solve_ref("e7", "c33_c2", False)
    c, h, origin = s["c"], s["h"], s["origin"]
    win = c["window"]
    sl = _put(ctx, c["T"])
    d = _data(s, rhs)
    kw = dict(t0=R.T0, window=win, damp=damp, max_iter=3)
    hn = h.copy()
    hn[5] = complex(np.nan, 0.0)
    bad = [
        lambda: ctx.tfm_lsq(sl, sl, d, R.FS, pulse=np.zeros(0), **kw),                      # ntap 0
        lambda: ctx.tfm_lsq(sl, sl, d, R.FS, pulse=np.ones(1025), **kw),                    # ntap 1025
        lambda: ctx.tfm_lsq(sl, sl, d, R.FS, pulse=h, pulse_origin=len(h), **kw),           # origin = ntap
        lambda: ctx.tfm_lsq(sl, sl, d, R.FS, pulse=h, pulse_origin=-1, **kw),
        lambda: ctx.tfm_lsq(sl, sl, d, R.FS, pulse=hn, pulse_origin=origin, **kw),          # a NaN tap
        lambda: ctx.tfm_lsq(sl, sl, d, R.FS, pulse=np.array([1.0, np.inf]), **kw),
        lambda: ctx.tfm_lsq(sl, sl, d, -R.FS, pulse=h, pulse_origin=origin, **kw),          # a condition of alifmm_tfm_lsq
        lambda: ctx.tfm_lsq(sl, sl, d, R.FS, pulse=h, pulse_origin=origin, **dict(kw, damp=-1.0)),
    ]
    # what only the C-ABI can express: complex taps with real data, tap_comp, a null pulse
    si = np.asarray(sl, dtype=np.int32)
    dc = L.as_samples64(d)
    d1 = np.ascontiguousarray(dc[..., 0])
    taps = np.ascontiguousarray(h).view(np.float64).reshape(-1, 2)
    img = np.full(win[2:] + (2,), 123.0)
    res = np.full(dc.shape, 123.0)
    info = np.full(8, 123.0)
    p = lambda a: None if a is None else a.ctypes.data

    def raw(data, ncomp, ntap, tap_comp, tp, org, image=img, max_iter=3, tol=1e-6):
        rc = _alifmm.lib().alifmm_tfm_lsq_pulse(ctx._h, 1, 7, p(si), 7, p(si), p(data), R.NT, ncomp, R.T0, R.FS, None, *win, 1,
                                                damp, 0.0, max_iter, tol, ntap, tap_comp, p(tp), org, p(image), p(res),
                                                p(info))
        ctx._chk(rc, "tfm_lsq_pulse")

    bad += [
        lambda: raw(d1, 1, 33, 2, taps, origin),      # complex taps with real data
        lambda: raw(dc, 2, 33, 0, taps, origin),      # tap_comp
        lambda: raw(dc, 2, 33, 3, taps, origin),
        lambda: raw(dc, 2, 33, 2, None, origin),      # null pointers
        lambda: raw(dc, 2, 33, 2, taps, origin, image=None),
        lambda: raw(dc, 2, 0, 2, taps, 0),            # ntap
        lambda: raw(dc, 2, 1025, 2, taps, origin),
        lambda: raw(dc, 2, 33, 2, taps, 33),          # origin
    ]
    for k, call in enumerate(bad):
        with pytest.raises(E, match="rc=-2"):
            call()
            pytest.fail("rejected input %d was accepted" % k)
    assert (img == 123.0).all() and (res == 123.0).all() and (info == 123.0).all()
    with pytest.raises(ValueError, match="complex pulse"):
        ctx.tfm_lsq(sl, sl, d.real, R.FS, pulse=h, pulse_origin=origin, **kw)
    with pytest.raises(ValueError):
        ctx.tfm_lsq(sl, sl, d, R.FS, pulse=np.ones((3, 3)), **kw)
    # the context is still usable: valid calls pass, raw and through Python
    raw(dc, 2, 33, 2, taps, origin, max_iter=1000, tol=1e-10)
    assert L.deviation(img.reshape(-1), xl) <= 8 * e_ref and info[5] == 0 and (res != 123.0).any()
    x, inf = _solve(ctx, s, rhs, damp=damp, max_iter=1000, tol=1e-10)
    assert L.deviation(_vec(s, x), xl) <= 8 * e_ref and inf["reason"] == "tol"


# ---- 9. the drop-in ----

def test_end_to_end_through_the_dropin(envelope):
    """ALI_FMM.lsq_image(pulse=h) inverts ALI_FMM.simulate_fmc(pulse=h) on computed fields (the 61²
    Voronoi model and 8 elements of test_gpu_tfm_lsq.py's drop-in test): three scatterers come back
    to 1e-2 (the restatement gives about 1e-5; the bar is loose because the host's FFT convolution
    and the device's direct sum differ by rounding, amplified by 1 / damp).  Without the pulse the
    same data leave more than half of their norm unexplained.  Measured on the MI355X: the map to
    1.9e-6 in 27 iterations; without the pulse 0.92 of the data's norm is left."""
    import Anis_TTF_rays as A

    n, dnx, fs = 61, 1e-3, R.FS
    veln = W.voronoi_small(n, seed=7)
    velpn = np.zeros((n, n), dtype=np.int64)
    vm = np.ones((n, n))
    sd = W.stif_field(n, n)
    xs = np.arange(6, 56, 7)
    Mo = A.ALI_FMM(veln, velpn, vm, dnx * xs.astype(float), np.zeros(8), stif_den=sd, dnx=dnx)
    F0 = Mo.update(veln, velpn, vm, sd)
    win = (20, 15, 12, 17)
    x_true = np.zeros(win[2:])
    x_true[3, 4], x_true[8, 11], x_true[8, 12] = 1.0, -0.5, 0.7
    h = F.pulse(17, 3, False)
    nt = math.ceil(2 * F0.max() * fs) + 2 + len(h)
    d = Mo.simulate_fmc(x_true, fs, nt, window=win, pulse=h)
    assert d.shape == (8, 8, nt) and d.any()
    # |A|_2 is of the order sqrt(ntx nrx) = 8 and |P|_2 of the order |h|_2: damp = 1e-3 of their product
    damp = 1e-3 * 8 * float(np.linalg.norm(h))
    img, info = Mo.lsq_image(d, fs, window=win, damp=damp, max_iter=500, tol=1e-8, pulse=h, pulse_origin=0)
    img0, info0 = Mo.lsq_image(d, fs, window=win, damp=damp, max_iter=500, tol=1e-8)
    e = {"x_error": L.deviation(img, x_true), "res_over_rhs": info["res_norm"] / info["rhs_norm"],
         "iterations": info["iterations"], "pulse_less_res_over_rhs": info0["res_norm"] / info0["rhs_norm"],
         "pulse_less_iterations": info0["iterations"]}
    envelope["tfm_lsq_pulse/dropin"] = e
    print("tfm_lsq_pulse/dropin", e)
    assert info["reason"] == "tol" and img.shape == win[2:] and img.dtype == np.float64
    assert e["x_error"] < 1e-2
    assert e["pulse_less_res_over_rhs"] > 0.5
    with pytest.raises(ValueError, match="complex pulse"):
        Mo.lsq_image(d, fs, window=win, pulse=F.pulse(17, 3, True))
