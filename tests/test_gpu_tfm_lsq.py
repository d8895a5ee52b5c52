"""GPU tests of least-squares imaging over resident fields (include/alifmm.h alifmm_tfm_f64 and
alifmm_tfm_lsq; csrc/tfm.hip in float64, csrc/tfm_solve.hip, csrc/tfm_model.hip inside the loop)
against the numpy restatement tests/tfm_lsq_ref.py.  The fields are uploaded with put_field after
set_model of the isotropic 37 x 70 model of test_gpu_tfm.py, so the kernels run on exactly known
delays.

Bars.  The float64 TFM: tfm_ref.bound with the float64 samples' magnitudes; the image of the
float32 cast of the same data misses that bar by at least tfm_lsq_ref.cast_gap (derived there: 3e4
at 7 x 7 pairs, 41 at 65 x 65; measured 4.0e5 to 6.8e5 and 586 to 632; a factor of 1e6 is out of
any data's reach at these pair counts, the bar growing with the pair count and the cast's error
with its square root, while the kernel itself stays below 2e-4 of the bar).  A solve at tol
1e-8: the true gradient of the stacked dense system is at most 2 tol |Bᵀ b|.  At tol 1e-10: within
8 e_ref of numpy's lstsq, e_ref being the restatement's own deviation from it (the margin
test_gpu_sens_solve.py grants another summation order), iterations within 1 of the restatement's,
|d|, |Aᵀ d| and the recurred |r| within 1e-9 of the restatement's, and the final gradient under the
stop rule (the final gamma itself is rounding noise of the iteration and differs between any two
summation orders).  A comparison of iterates after a fixed number of iterations is relative to the
iterate's norm, 1e-11.  A sums with atomics: no test asserts bit equality between two solves.  The
measured figures go to the session's envelope under tfm_lsq/... ."""
import math

import numpy as np
import pytest

import tfm_lsq_ref as L
import tfm_model_ref as M
import tfm_ref as R
import workloads as W

pytestmark = pytest.mark.gpu

FULL = R.full_window((R.NZ, R.NX))


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    c.set_model(np.zeros((R.NZ, R.NX)), np.ones((R.NZ, R.NX), dtype=np.int64), np.full((R.NZ, R.NX), R.SPEED), None,
                W.default_table(), W.default_table(), R.DNX)
    yield c
    c.close()


def _put(ctx, T, first=0, subgrid=1):
    for k, f in enumerate(T):
        ctx.put_field(first + k, subgrid, f)
    return list(range(first, first + len(T)))


def _close(x, ref, rtol=1e-11):
    """|x - ref| <= rtol |ref| over the whole array."""
    return np.linalg.norm(np.asarray(x) - ref) <= rtol * np.linalg.norm(ref)


# ---- 1. the float64 TFM against the restatement ----

@pytest.mark.parametrize("n,ncomp", [(7, 1), (7, 2), (65, 1), (65, 2)])
def test_f64_against_the_restatement(ctx, envelope, n, ncomp):
    """7 elements (one partial chunk) and 65 (many chunks and a partial one), real and complex, the
    full window, a window aligned to nothing and step 3, every tfm_chunk; float64 noise that float32
    does not represent."""
    T = R.fields(R.element_x(n))
    s = _put(ctx, T)
    d = L.noise64(n, n, ncomp=ncomp)
    d32 = d.astype(np.complex64 if ncomp == 2 else np.float32)
    try:
        for name, win, step in (("full", FULL, 1), ("window", R.WINDOW, 1), ("step3", R.WINDOW_STEP3, 3)):
            ref, mag = L.tfm_f64_ref(T, T, d, R.FS, R.T0, None, win, step)
            cast, _ = L.tfm_f64_ref(T, T, d32, R.FS, R.T0, None, win, step)
            gap = R.worst_ratio(cast, ref, n * n, mag)
            assert gap > L.cast_gap(n * n), (name, gap)  # the bar tells the two kernels apart
            for chunk in (4, 8, 16, 32):
                ctx.set_option("tfm_chunk", chunk)
                img = ctx.tfm(s, s, d, R.FS, t0=R.T0, window=None if win == FULL and step == 1 else win, step=step,
                              precision="f64")
                assert img.shape == ref.shape and img.dtype == ref.dtype
                r = R.worst_ratio(img, ref, n * n, mag)
                key = "tfm_lsq/f64_n%d_c%d_%s_chunk%d" % (n, ncomp, name, chunk)
                envelope[key] = r
                print("%s: worst |I - I_ref| / bound = %.3g (the float32 cast: %.3g)" % (key, r, gap))
                assert r <= 1.0, (key, r)
                assert np.all(img[mag == 0] == 0)
    finally:
        ctx.set_option("tfm_chunk", 8)


# ---- 2. bit properties ----

@pytest.mark.parametrize("ncomp", [1, 2])
def test_f64_bits(ctx, ncomp):
    """On float32-representable data the float64 call has the bits of the float32 call at the same
    chunk; two float64 calls have equal bits; a pixel has the same bits through two windows."""
    n = 65
    T = R.fields(R.element_x(n))
    s = _put(ctx, T)
    d32 = R.data(n, n, ncomp=ncomp)
    d = L.noise64(n, n, ncomp=ncomp)
    try:
        for chunk in (8, 16):
            ctx.set_option("tfm_chunk", chunk)
            a = ctx.tfm(s, s, d32, R.FS, t0=R.T0)
            b = ctx.tfm(s, s, d32.astype(np.complex128 if ncomp == 2 else np.float64), R.FS, t0=R.T0, precision="f64")
            assert a.any() and np.array_equal(a, b)
            full = ctx.tfm(s, s, d, R.FS, t0=R.T0, precision="f64")
            assert np.array_equal(full, ctx.tfm(s, s, d, R.FS, t0=R.T0, precision="f64"))
            assert not np.array_equal(full, ctx.tfm(s, s, d, R.FS, t0=R.T0))  # the float32 call truncates these data
            i0, j0, ni, nj = R.WINDOW
            win = ctx.tfm(s, s, d, R.FS, t0=R.T0, window=R.WINDOW, precision="f64")
            assert np.array_equal(win, full[i0:i0 + ni, j0:j0 + nj])
            i0, j0, ni, nj = R.WINDOW_STEP3
            win = ctx.tfm(s, s, d, R.FS, t0=R.T0, window=R.WINDOW_STEP3, step=3, precision="f64")
            assert np.array_equal(win, full[i0:i0 + 3 * ni:3, j0:j0 + 3 * nj:3])
    finally:
        ctx.set_option("tfm_chunk", 8)
    with pytest.raises(ValueError, match="precision"):
        ctx.tfm(s, s, d32, R.FS, precision="f16")


# ---- 3., 4. solves ----

_refs = {}


def _solve_ref(name, ncomp, smooth_on):
    key = (name, ncomp, smooth_on)
    if key not in _refs:
        c, rhs, damp, smooth = L.problem(name, ncomp, smooth_on)
        xl = L.lstsq(c["A"], c["D"], rhs, damp, smooth)
        x10, i10, _ = L.cgls(c["A"], c["D"], rhs, damp, smooth, 1000, 1e-10)
        x8, i8, _ = L.cgls(c["A"], c["D"], rhs, damp, smooth, 1000, 1e-8)
        _refs[key] = (c, rhs, damp, smooth, xl, L.deviation(x10, xl), i10, i8)
    return _refs[key]


def _solve(ctx, c, rhs, **kw):
    s = _put(ctx, c["T"])
    return ctx.tfm_lsq(s, s, L.data_of(c, rhs), R.FS, t0=R.T0, window=c["window"], step=c["step"], **kw)


def _check_solve(ctx, envelope, name, ncomp, smooth_on):
    c, rhs, damp, smooth, xl, e_ref, i10, i8 = _solve_ref(name, ncomp, smooth_on)
    x8, info8 = _solve(ctx, c, rhs, damp=damp, smooth=smooth, max_iter=1000, tol=1e-8)
    assert x8.shape == c["window"][2:] and x8.dtype == (np.complex128 if ncomp == 2 else np.float64)
    g, g0 = L.true_gradient(c["A"], c["D"], rhs, damp, smooth, L.columns(x8))
    x10, info10 = _solve(ctx, c, rhs, damp=damp, smooth=smooth, max_iter=1000, tol=1e-10)
    e_gpu = L.deviation(L.columns(x10), xl)
    key = "tfm_lsq/solve_%s_c%d%s" % (name, ncomp, "_smooth" if smooth_on else "")
    envelope[key] = {"true_gradient_over_BTb_tol1e-8": g / g0, "e_gpu_tol1e-10": e_gpu, "e_ref_tol1e-10": e_ref,
                     "iterations_gpu": [info8["iterations"], info10["iterations"]],
                     "iterations_ref": [i8["iterations"], i10["iterations"]],
                     "tfm_lsq_kernel_ms": ctx.get_option("tfm_lsq_kernel_ms")}
    print(key, envelope[key])
    assert info8["reason"] == "tol" and info10["reason"] == "tol"
    assert g <= 2 * 1e-8 * g0, (g, g0)
    assert e_gpu <= 8 * e_ref, (e_gpu, e_ref)
    assert abs(info8["iterations"] - i8["iterations"]) <= 1
    assert abs(info10["iterations"] - i10["iterations"]) <= 1
    assert ctx.get_option("tfm_lsq_iters") == info10["iterations"]
    assert ctx.get_option("tfm_lsq_kernel_ms") > 0 and ctx.get_option("tfm_lsq_upload_ms") > 0
    for got, want in ((info10["rhs_norm"], i10["rhs_norm"]), (info10["grad0"], i10["grad0"]),
                      (info10["res_norm"], i10["res_norm"])):
        assert abs(got - want) <= 1e-9 * want, (got, want)
    assert info10["grad"] <= 1e-10 * info10["grad0"]


@pytest.mark.parametrize("ncomp", [1, 2])
@pytest.mark.parametrize("name", list(L.CASES))
def test_solve(ctx, envelope, name, ncomp):
    _check_solve(ctx, envelope, name, ncomp, False)


@pytest.mark.parametrize("name,ncomp", [("e7s3", 2), ("e1", 1)])
def test_solve_smooth(ctx, envelope, name, ncomp):
    """smooth = damp: the stencil on a 10 x 20 window at step 3 (complex: a component stride of 2)
    and on the rank-deficient one-element case, against the stacked lstsq."""
    _check_solve(ctx, envelope, name, ncomp, True)


# ---- 5. the paths of the modelling kernel inside the loop ----

def test_model_paths_in_the_loop(ctx, envelope):
    """Three iterations against the restatement's three, relative to the iterate's norm: automatic
    slabs > 1 (one element on the full window: the automatic rule gives a slab per 1024 pixels, so
    the 9 x 13 window of the solve cases stays at one; q is zeroed every iteration and flushed with
    atomics), tfm_model_slabs 1 and 4 and tfm_model_tile 64 (time tiles) on the 7-element case,
    and nt = 5000 complex with 3 elements (two LDS passes)."""
    def three(name, T, d, fs, window, step, A, D, damp):
        s = _put(ctx, T)
        x, info = ctx.tfm_lsq(s, s, d, fs, t0=R.T0, window=window, step=step, damp=damp, smooth=damp, max_iter=3, tol=0.0)
        xr, ir, _ = L.cgls(A, D, L.columns(d), damp, damp, 3, 0.0)
        e = np.linalg.norm(L.columns(x) - xr) / np.linalg.norm(xr)
        envelope["tfm_lsq/three_" + name] = e
        print("tfm_lsq/three_%s: |x - x_ref| / |x_ref| = %.3g, slabs %d, tile %d" %
              (name, e, ctx.get_option("tfm_model_slabs_used"), ctx.get_option("tfm_model_tile_used")))
        assert info["iterations"] == 3 and info["reason"] == "max_iter"
        assert e <= 1e-11, (name, e)

    T1 = R.fields(R.element_x(1))
    A1 = L.dense_A(T1, T1, R.NT, R.FS, R.T0)
    D1 = L.difference(*FULL[2:])
    rng = np.random.default_rng(50)
    d1 = L.from_columns(A1 @ rng.standard_normal((A1.shape[1], 2)) + 0.01 * rng.standard_normal((A1.shape[0], 2)),
                        (1, 1, R.NT))
    three("auto_slabs", T1, d1, R.FS, FULL, 1, A1, D1, 0.02)
    assert ctx.get_option("tfm_model_slabs_used") > 1
    c, rhs, damp, _ = L.problem("e7", 2)
    d7 = L.data_of(c, rhs)
    try:
        for slabs in (1, 4):
            ctx.set_option("tfm_model_slabs", slabs)
            three("slabs%d" % slabs, c["T"], d7, R.FS, c["window"], c["step"], c["A"], c["D"], damp)
            assert ctx.get_option("tfm_model_slabs_used") == slabs
        ctx.set_option("tfm_model_slabs", 0)
        ctx.set_option("tfm_model_tile", 64)
        three("tile64", c["T"], d7, R.FS, c["window"], c["step"], c["A"], c["D"], damp)
        assert ctx.get_option("tfm_model_tile_used") == 64
    finally:
        ctx.set_option("tfm_model_slabs", 0)
        ctx.set_option("tfm_model_tile", 0)
    T3 = R.fields(R.element_x(3))
    fs = 5000 / 480 * R.FS
    win = L.CASES["e7"][1]
    A3 = L.dense_A(T3, T3, 5000, fs, R.T0, None, win, 1)
    assert A3[:, :].reshape(9, 5000, -1)[:, 4096:].any() and A3.reshape(9, 5000, -1)[:, :4096].any()
    d3 = L.from_columns(A3 @ rng.standard_normal((A3.shape[1], 2)) + 0.01 * rng.standard_normal((A3.shape[0], 2)),
                        (3, 3, 5000))
    three("nt5000", T3, d3, fs, win, 1, A3, L.difference(*win[2:]), 0.05)
    assert ctx.get_option("tfm_model_tile_used") == 4096


# ---- 6. the residual ----

@pytest.mark.parametrize("ncomp", [1, 2])
def test_resid(ctx, ncomp):
    c, rhs, damp, smooth, xl, e_ref, i10, i8 = _solve_ref("e7s3", ncomp, False)
    x, info, res = _solve(ctx, c, rhs, damp=damp, max_iter=1000, tol=1e-8, resid=True)
    d = L.data_of(c, rhs)
    assert res.shape == d.shape and res.dtype == d.dtype
    want = rhs - c["A"] @ L.columns(x)
    err = np.abs(L.columns(res) - want).max()
    print("resid c%d: max |r - (b - A x)| = %.3g, |b| = %.3g" % (ncomp, err, info["rhs_norm"]))
    assert err <= 1e-12 * info["rhs_norm"]
    assert abs(info["res_norm"] - np.linalg.norm(L.columns(res))) <= 1e-12 * info["res_norm"]
    assert info["res_norm"] < info["rhs_norm"]


# ---- 7. stops and errors ----

def test_stops(ctx):
    c, rhs, damp, _ = L.problem("e7", 2)
    d = L.data_of(c, rhs)
    for z in (np.zeros_like(d), np.zeros(d.shape)):
        x, info = _solve(ctx, c, L.columns(z), damp=damp, smooth=damp, max_iter=10, tol=1e-8)
        parts = (x.real, x.imag) if np.iscomplexobj(x) else (x,)
        assert info["reason"] == "breakdown" and info["iterations"] == 0
        assert all(not p.any() and not np.signbit(p).any() for p in parts)
        assert info["grad0"] == 0 and info["rhs_norm"] == 0 and info["res_norm"] == 0
    x, info = _solve(ctx, c, rhs, damp=damp, smooth=damp, max_iter=1, tol=1e-8)
    xr, _, _ = L.cgls(c["A"], c["D"], rhs, damp, damp, 1, 1e-8)
    assert info["reason"] == "max_iter" and info["iterations"] == 1
    assert x.any() and _close(L.columns(x), xr)


def test_slots_untouched(ctx):
    c, rhs, damp, _ = L.problem("e7", 2)
    s = _put(ctx, c["T"])
    before = [ctx.get_field(k, 1) for k in s]
    _solve(ctx, c, rhs, damp=damp, max_iter=5)
    for k in s:
        assert np.array_equal(ctx.get_field(k, 1), before[k]) and np.array_equal(before[k], c["T"][k])


def _raw(ctx, subgrid, tx, rx, fmc, nt, ncomp, t0, fs, w, win, step, damp, smooth, max_iter, tol, image, resid, info):
    """alifmm_tfm_lsq as declared, for the arguments the Python layer cannot express."""
    import _alifmm

    p = lambda a: None if a is None else a.ctypes.data
    rc = _alifmm.lib().alifmm_tfm_lsq(ctx._h, subgrid, len(tx) if tx is not None else 1, p(tx),
                                      len(rx) if rx is not None else 1, p(rx), p(fmc), nt, ncomp, t0, fs, p(w), *win, step,
                                      damp, smooth, max_iter, tol, p(image), p(resid), p(info))
    ctx._chk(rc, "tfm_lsq")


def test_errors(ctx, envelope):
    """Every rejected input of the contract raises with rc=-2 and leaves the outputs as they were;
    a valid call passes afterwards."""
    import _alifmm

    E = _alifmm.AlifmmError
    c, rhs, damp, smooth, xl, e_ref, i10, i8 = _solve_ref("e7", 2, False)
    T, win = c["T"], c["window"]
    s = _put(ctx, T)
    ctx.put_field(7, 3, np.zeros((109, 208)))
    d = L.data_of(c, rhs)
    kw = dict(t0=R.T0, window=win, damp=damp, max_iter=3)
    bare = _alifmm.Context(0)
    with pytest.raises(E, match="no model"):
        bare.tfm_lsq([0], [0], d[:1, :1], R.FS, window=win)
    bare.close()
    dn, di = d.copy(), d.copy()
    dn[6, 6, R.NT - 1] = complex(0.0, np.nan)
    di[0, 0, 0] = -np.inf

    def but(**over):
        k = dict(kw)
        k.update(over)
        return k

    bad = [
        lambda: ctx.tfm_lsq([0, 999] + s[2:], s, d, R.FS, **kw),            # empty slot
        lambda: ctx.tfm_lsq(s, [-1] + s[1:], d, R.FS, **kw),
        lambda: ctx.tfm_lsq(s, s[:6] + [7], d, R.FS, **kw),                 # mixed subgrids and shapes
        lambda: ctx.tfm_lsq(s, s, d, R.FS, subgrid=3, **kw),                # not the fields' subgrid
        lambda: ctx.tfm_lsq([], s, d[:0], R.FS, **kw),                      # ntx < 1
        lambda: ctx.tfm_lsq(s, [], d[:, :0], R.FS, **kw),                   # nrx < 1
        lambda: ctx.tfm_lsq(s, s, d[:, :, :1], R.FS, **kw),                 # nt < 2
        lambda: ctx.tfm_lsq(s, s, d, 0.0, **kw),                            # fs
        lambda: ctx.tfm_lsq(s, s, d, -R.FS, **kw),
        lambda: ctx.tfm_lsq(s, s, d, math.nan, **kw),
        lambda: ctx.tfm_lsq(s, s, d, math.inf, **kw),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(t0=math.nan)),             # t0
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(t0=-math.inf)),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, step=0, **kw),                   # step, niz, nix
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(window=None), step=0),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(window=(0, 0, 0, 5))),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(window=(0, 0, 5, 0))),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(window=(0, 0, R.NZ + 1, R.NX))),  # outside
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(window=(0, 0, R.NZ, R.NX + 1))),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(window=(-1, 0, 5, 5))),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(window=(0, -1, 5, 5))),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, step=3, **but(window=(1, 2, 13, 23))),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, step=2 ** 30, **but(window=(5, 5, 2, 2))),
        lambda: ctx.tfm_lsq(s, s, dn, R.FS, **kw),                          # non-finite data
        lambda: ctx.tfm_lsq(s, s, di, R.FS, **kw),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(damp=-1.0)),               # damp, smooth, max_iter, tol
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(damp=math.nan)),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(damp=math.inf)),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, smooth=-1e-9, **kw),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, smooth=math.nan, **kw),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, smooth=math.inf, **kw),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, **but(max_iter=0)),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, tol=-1e-3, **kw),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, tol=math.nan, **kw),
        lambda: ctx.tfm_lsq(s, s, d, R.FS, tol=math.inf, **kw),
    ]
    # the arguments only the C-ABI can express: ncomp, null pointers; the outputs stay as they were
    si = np.asarray(s, dtype=np.int32)
    dc = L.as_samples64(d)
    img = np.full(win[2:] + (2,), 123.0)
    res = np.full(dc.shape, 123.0)
    info = np.full(8, 123.0)
    tail = (damp, 0.0, 3, 1e-6)
    bad += [
        lambda: _raw(ctx, 1, si, si, dc, R.NT, 3, R.T0, R.FS, None, win, 1, *tail, img, res, info),
        lambda: _raw(ctx, 1, si, si, dc, R.NT, 0, R.T0, R.FS, None, win, 1, *tail, img, res, info),
        lambda: _raw(ctx, 1, None, si, dc, R.NT, 2, R.T0, R.FS, None, win, 1, *tail, img, res, info),
        lambda: _raw(ctx, 1, si, None, dc, R.NT, 2, R.T0, R.FS, None, win, 1, *tail, img, res, info),
        lambda: _raw(ctx, 1, si, si, None, R.NT, 2, R.T0, R.FS, None, win, 1, *tail, img, res, info),
        lambda: _raw(ctx, 1, si, si, dc, R.NT, 2, R.T0, R.FS, None, win, 1, *tail, None, res, info),
        lambda: _raw(ctx, 1, si, si, dc, R.NT, 2, R.T0, R.FS, None, win, 1, *tail, img, res, None),
        lambda: _raw(ctx, 1, si, si, L.as_samples64(dn), R.NT, 2, R.T0, R.FS, None, win, 1, *tail, img, res, info),
        lambda: _raw(ctx, 1, si, si, dc, R.NT, 2, R.T0, R.FS, None, (5, 5, 2 ** 31 - 1, 2), 2 ** 31 - 1, *tail, img, res, info),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(E, match="rc=-2|tfm_lsq: step"):
            call()
            pytest.fail("rejected input %d was accepted" % k)
    assert (img == 123.0).all() and (res == 123.0).all() and (info == 123.0).all()
    # the same through tfm(precision="f64"): alifmm_tfm's errors
    for call in (lambda: ctx.tfm(s, s[:6] + [7], d, R.FS, precision="f64"),
                 lambda: ctx.tfm(s, s, d, -R.FS, precision="f64"),
                 lambda: ctx.tfm(s, s, d, R.FS, window=(0, 0, R.NZ + 1, R.NX), precision="f64")):
        with pytest.raises(E, match="rc=-2"):
            call()
    # the Python layer's own checks
    with pytest.raises(ValueError):
        ctx.tfm_lsq(s, s, d[:5], R.FS, **kw)
    with pytest.raises(ValueError):
        ctx.tfm_lsq(s, s, d, R.FS, weights=np.ones((7, 6)), **kw)
    # the context is still usable: valid calls pass, raw (without a residual) and through Python
    _raw(ctx, 1, si, si, dc, R.NT, 2, R.T0, R.FS, None, win, 1, damp, 0.0, 1000, 1e-10, img, None, info)
    assert L.deviation(img.reshape(-1, 2), xl) <= 8 * e_ref and info[5] == 0 and (res == 123.0).all()
    x, inf = ctx.tfm_lsq(s, s, d, R.FS, t0=R.T0, window=win, damp=damp, max_iter=1000, tol=1e-10)
    assert L.deviation(L.columns(x), xl) <= 8 * e_ref and inf["reason"] == "tol"


def test_weights(ctx, envelope):
    """Pair weights with zeros and negative values reach both products: three iterations against
    the restatement on the weighted operator."""
    c, rhs, damp, _ = L.problem("e7", 2)
    rng = np.random.default_rng(8)
    w = rng.standard_normal((7, 7)).astype(np.float32)
    w[rng.random((7, 7)) < 0.3] = 0
    assert 0 < (w == 0).sum() < 49 and (w < 0).any()
    Aw = c["A"] * np.repeat(w.astype(np.float64).ravel(), R.NT)[:, None]
    s = _put(ctx, c["T"])
    d = L.data_of(c, rhs)
    x, info = ctx.tfm_lsq(s, s, d, R.FS, t0=R.T0, weights=w, window=c["window"], damp=damp, max_iter=3, tol=0.0)
    xr, _, _ = L.cgls(Aw, c["D"], rhs, damp, 0.0, 3, 0.0)
    e = np.linalg.norm(L.columns(x) - xr) / np.linalg.norm(xr)
    envelope["tfm_lsq/three_weights"] = e
    assert info["iterations"] == 3 and e <= 1e-11, e


# ---- 8. reproducibility ----

def test_reproducibility(ctx, envelope):
    """Two solves of the 2-element case agree within 8 e_ref of each other; bit equality is not
    promised and not asserted."""
    c, rhs, damp, smooth, xl, e_ref, i10, i8 = _solve_ref("e2", 2, False)
    x1, i1 = _solve(ctx, c, rhs, damp=damp, max_iter=1000, tol=1e-10)
    x2, i2 = _solve(ctx, c, rhs, damp=damp, max_iter=1000, tol=1e-10)
    e = L.deviation(L.columns(x2), L.columns(x1))
    envelope["tfm_lsq/repeat"] = {"deviation": e, "e_ref": e_ref, "iterations": [i1["iterations"], i2["iterations"]]}
    print("tfm_lsq/repeat", envelope["tfm_lsq/repeat"])
    assert e <= 8 * e_ref and abs(i1["iterations"] - i2["iterations"]) <= 1


# ---- 9. the drop-in ----

def test_end_to_end_through_the_dropin(envelope):
    """ALI_FMM.lsq_image on computed fields (the 61² Voronoi model and 8 elements of
    test_gpu_tfm_model.py::test_end_to_end_through_the_dropin): the data of a sparse map on a
    window; the image equals Context.tfm_lsq on the named slots within the reproducibility bar, its
    residual norm is below |d| and is that of simulate_fmc(image).  The same with the transmit path
    reflected off the last row."""
    import Anis_TTF_rays as A

    n, dnx, fs = 61, 1e-3, R.FS
    veln = W.voronoi_small(n, seed=7)
    velpn = np.zeros((n, n), dtype=np.int64)
    vm = np.ones((n, n))
    sd = W.stif_field(n, n)
    xs = np.arange(6, 56, 7)
    Mo = A.ALI_FMM(veln, velpn, vm, dnx * xs.astype(float), np.zeros(8), stif_den=sd, dnx=dnx)
    F = Mo.update(veln, velpn, vm, sd)
    win = (20, 15, 12, 17)
    x_true = np.zeros(win[2:])
    x_true[3, 4], x_true[8, 11], x_true[8, 12] = 1.0, -0.5, 0.7
    wall = np.full(n, n - 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    c = Mo._ctx(0)
    for name, kw in (("direct", {}), ("half_skip", dict(tx_path="skip", reflector=wall))):
        # the fields computed and left on the device, and the slots that name them
        txs, rxs = Mo._pair_slots("lsq_image", None, None, 1, None, None, None, None, kw.get("tx_path", "direct"),
                                  "direct", kw.get("reflector"))
        Tt = np.stack([c.get_field(k, 1) for k in txs])
        Tr = np.stack([c.get_field(k, 1) for k in rxs])
        assert np.isfinite(Tt).all() and (kw or np.array_equal(Tt, F))
        nt = math.ceil((Tt.max() + Tr.max()) * fs) + 2
        d = Mo.simulate_fmc(x_true, fs, nt, window=win, **kw)
        assert d.any()
        damp = 1e-2 * 8
        img, info = Mo.lsq_image(d, fs, window=win, damp=damp, max_iter=200, tol=1e-10, **kw)
        Ad = L.dense_A(Tt, Tr, nt, fs, 0.0, None, win, 1)
        Dd = L.difference(*win[2:])
        rhs = L.columns(d)
        xl = L.lstsq(Ad, Dd, rhs, damp, 0.0)
        xr, ir, _ = L.cgls(Ad, Dd, rhs, damp, 0.0, 200, 1e-10)
        e_ref = L.deviation(xr, xl)
        e = L.deviation(L.columns(img), xl)
        img2, info2 = c.tfm_lsq(txs, rxs, d, fs, window=win, damp=damp, max_iter=200, tol=1e-10)
        e2 = L.deviation(L.columns(img2), L.columns(img))
        assert e2 <= 8 * e_ref, (e2, e_ref)
        envelope["tfm_lsq/dropin_" + name] = {"e_gpu": e, "e_ref": e_ref, "e_repeat": e2, "iterations": info["iterations"],
                                              "iterations_ref": ir["iterations"]}
        print("tfm_lsq/dropin_" + name, envelope["tfm_lsq/dropin_" + name])
        assert info["reason"] == "tol" and img.shape == win[2:] and img.dtype == np.float64
        assert e <= 8 * e_ref, (e, e_ref)
        assert info["res_norm"] < info["rhs_norm"] and abs(info["rhs_norm"] - np.linalg.norm(d)) <= 1e-12 * info["rhs_norm"]
        back = np.linalg.norm(d - Mo.simulate_fmc(img, fs, nt, window=win, **kw))
        assert abs(info["res_norm"] - back) <= 1e-6 * back, (info["res_norm"], back)
    with pytest.raises(IndexError, match="lsq_image"):
        Mo.lsq_image(d, fs, window=win, tx=[8])
    with pytest.raises(ValueError, match="lsq_image"):
        Mo.lsq_image(d, fs, window=win, tx_path="skip")
