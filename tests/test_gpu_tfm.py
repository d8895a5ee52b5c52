"""GPU tests of the TFM delay-and-sum over resident fields (include/alifmm.h alifmm_tfm, csrc/tfm.hip)
against the numpy restatement of its contract (tests/tfm_ref.py).  The fields are uploaded with
put_field after set_model of an isotropic 37 x 70 model, so the kernel runs on exactly known delays.

The bar of every comparison, per pixel and component: |I - I_ref| <= 2 (npairs + 4) 2^-53 A(p),
A(p) = sum |w| (|x0| + |x1|) over the in-range terms.  It is derived, not measured: a term carries
three float64 roundings of magnitude <= |w| (|x0| + |x1|), and a sum of n terms in any order adds at
most (n - 1) 2^-53 sum |term|.  Delays rounded to float32 exceed it by 10^9 or more.  Where A(p) is 0
(no term in range) the image must be exactly 0.  The worst measured ratio of each case goes to the
session's envelope under tfm/... ."""
import ctypes
import math

import numpy as np
import pytest

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


_cache = {}


def _case(n, ncomp):
    """Fields, data and the full-window reference of n elements (computed once, never modified)."""
    key = (n, ncomp)
    if key not in _cache:
        T = R.fields(R.element_x(n))
        fmc = R.data(n, n, ncomp=ncomp)
        ref, mag, _ = R.tfm_ref(T, T, fmc, R.FS, R.T0)
        for a in (T, fmc, ref, mag):
            a.setflags(write=False)
        _cache[key] = (T, fmc, ref, mag)
    return _cache[key]


def _put(ctx, T, first=0, subgrid=1):
    for k, f in enumerate(T):
        ctx.put_field(first + k, subgrid, f)
    return list(range(first, first + len(T)))


def _sub(a, window, step=1):
    z, x, nz, nx = window
    return a[z:z + step * nz:step, x:x + step * nx:step]


def _check(envelope, name, img, ref, npairs, mag):
    assert img.shape == ref.shape and img.dtype == ref.dtype
    r = R.worst_ratio(img, ref, npairs, mag)
    envelope["tfm/" + name] = r
    print("tfm/%s: worst |I - I_ref| / bound = %.3g" % (name, r))
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("n,ncomp", [(1, 2), (7, 2), (65, 2), (130, 2), (7, 1)])
def test_element_counts(ctx, envelope, n, ncomp):
    """65 and 130 cross the receiver chunk (8) with a partial last chunk, 1 and 7 stay inside one;
    full window (tail tiles in x and z) and a window aligned to no tile."""
    T, fmc, ref, mag = _case(n, ncomp)
    s = _put(ctx, T)
    img = ctx.tfm(s, s, fmc, R.FS, t0=R.T0)
    _check(envelope, "n%d_c%d_full" % (n, ncomp), img, ref, n * n, mag)
    win = ctx.tfm(s, s, fmc, R.FS, t0=R.T0, window=R.WINDOW)
    _check(envelope, "n%d_c%d_window" % (n, ncomp), win, _sub(ref, R.WINDOW), n * n, _sub(mag, R.WINDOW))


def test_chunk_option(ctx, envelope):
    """Every value of option tfm_chunk (another summation order, the same bar); 65 receivers leave
    a partial last chunk for each.  The default gives the bits of test_element_counts again."""
    T, fmc, ref, mag = _case(65, 2)
    s = _put(ctx, T)
    default = int(ctx.get_option("tfm_chunk"))
    base = ctx.tfm(s, s, fmc, R.FS, t0=R.T0)
    try:
        for c in (4, 8, 16, 32):
            ctx.set_option("tfm_chunk", c)
            img = ctx.tfm(s, s, fmc, R.FS, t0=R.T0)
            _check(envelope, "chunk%d" % c, img, ref, 65 * 65, mag)
            assert (c != default) or np.array_equal(img, base)
    finally:
        ctx.set_option("tfm_chunk", default)
    with pytest.raises(Exception):
        ctx.set_option("tfm_chunk", 5)
    assert int(ctx.get_option("tfm_chunk")) == default


def test_slot_lists(ctx, envelope):
    """ntx 5 against nrx 9; tx reversed with one slot repeated, rx a strided subset, slots not
    starting at 0: a swapped or transposed index shows."""
    T = R.fields(R.element_x(24))
    _put(ctx, T, first=3)
    tx = [3 + e for e in (20, 11, 11, 4, 1)]
    rx = list(range(3 + 2, 3 + 2 + 18, 2))
    fmc = R.data(5, 9, seed=6)
    img = ctx.tfm(tx, rx, fmc, R.FS, t0=R.T0)
    ref, mag, _ = R.tfm_ref(T[[s - 3 for s in tx]], T[[s - 3 for s in rx]], fmc, R.FS, R.T0)
    _check(envelope, "slot_lists", img, ref, 45, mag)
    swapped, _, _ = R.tfm_ref(T[[s - 3 for s in rx]][:5], T[[s - 3 for s in tx] + [0] * 4], fmc, R.FS, R.T0)
    assert R.worst_ratio(swapped, ref, 45, mag) > 1e6  # the reference itself tells the lists apart


def test_weights(ctx, envelope):
    T, fmc, _, _ = _case(7, 2)
    s = _put(ctx, T)
    rng = np.random.default_rng(8)
    w = rng.standard_normal((7, 7)).astype(np.float32)
    w[rng.random((7, 7)) < 0.3] = 0
    assert 0 < (w == 0).sum() < 49
    img = ctx.tfm(s, s, fmc, R.FS, t0=R.T0, weights=w)
    ref, mag, cnt = R.tfm_ref(T, T, fmc, R.FS, R.T0, w)
    assert cnt["zero_weight"] > 0
    _check(envelope, "weights", img, ref, 49, mag)
    zero = ctx.tfm(s, s, fmc, R.FS, t0=R.T0, weights=np.zeros((7, 7)))
    assert zero.shape == (R.NZ, R.NX) and not zero.real.any() and not zero.imag.any()


def test_nonfinite_fields(ctx, envelope):
    """NaN, +inf, -1.0 and 1e300 patches: every pair touching them contributes exactly 0 at those
    pixels (where every field is patched the image is exactly 0), the rest stays within the bar."""
    T0, fmc, _, _ = _case(7, 2)
    T = T0.copy()
    bad = [np.nan, np.inf, -1.0, 1e300]
    T[0, 5:8, 10:14] = np.nan
    T[2, 20:30, 60:70] = -1.0
    T[3, 0:4, 0:70] = 1e300
    T[5, 30:37, 0:9] = np.inf
    for e in range(7):  # every field patched here, by one of the four values
        T[e, 12:16, 30:41] = bad[e % 4]
    s = _put(ctx, T)
    w = np.ones((7, 7), dtype=np.float32)
    w[0, 3] = 0  # a zero weight on a NaN delay
    for name, wt in (("nonfinite", None), ("nonfinite_w", w)):
        img = ctx.tfm(s, s, fmc, R.FS, t0=R.T0, weights=wt)
        ref, mag, cnt = R.tfm_ref(T, T, fmc, R.FS, R.T0, wt)
        assert cnt["nonfinite"] > 0 and cnt["below"] > 0 and cnt["above"] > 0
        assert not mag[12:16, 30:41].any() and mag[5:8, 10:14].all()
        assert np.all(img[12:16, 30:41] == 0) and np.isfinite(img.real).all() and np.isfinite(img.imag).all()
        _check(envelope, name, img, ref, 49, mag)


def test_step_and_shape(ctx, envelope):
    T, fmc, ref, mag = _case(7, 2)
    s = _put(ctx, T)
    img = ctx.tfm(s, s, fmc, R.FS, t0=R.T0, window=R.WINDOW_STEP3, step=3)
    _check(envelope, "step3", img, _sub(ref, R.WINDOW_STEP3, 3), 49, _sub(mag, R.WINDOW_STEP3, 3))
    img = ctx.tfm(s, s, fmc, R.FS, t0=R.T0, step=3)  # window None: the whole field at that step
    _check(envelope, "step3_full", img, ref[::3, ::3], 49, mag[::3, ::3])
    small = (34, 66, 2, 3)
    img = ctx.tfm(s, s, fmc, R.FS, t0=R.T0, window=small)
    _check(envelope, "window_2x3", img, _sub(ref, small), 49, _sub(mag, small))
    # nt = 2: only u in [0, 1) is in range
    d2 = R.data(7, 7, nt=2, seed=9)
    fs, t0 = 1.2e5, 2e-6
    img = ctx.tfm(s, s, d2, fs, t0=t0)
    r2, m2, cnt = R.tfm_ref(T, T, d2, fs, t0)
    assert cnt["inside"] > 0 and cnt["below"] > 0 and cnt["above"] > 0
    _check(envelope, "nt2", img, r2, 49, m2)
    # subgrid 3: fine shape 109 x 208
    assert ctx.field_shape(3) == (109, 208)
    T3 = R.fields(3 * R.element_x(7), nz=109, nx=208, dnx=R.DNX / 3)
    s3 = _put(ctx, T3, first=7, subgrid=3)
    img = ctx.tfm(s3, s3, fmc, R.FS, t0=R.T0, subgrid=3)
    r3, m3, _ = R.tfm_ref(T3, T3, fmc, R.FS, R.T0)
    _check(envelope, "subgrid3", img, r3, 49, m3)
    w3 = (5, 7, 33, 65)
    win = ctx.tfm(s3, s3, fmc, R.FS, t0=R.T0, subgrid=3, window=w3, step=3)
    assert np.array_equal(win, _sub(img, w3, 3))


def test_determinism(ctx):
    """The same call twice gives the same bits, and a pixel has the same bits through every window
    and step (the summation order is fixed per pixel)."""
    T, fmc, _, _ = _case(65, 2)
    s = _put(ctx, T)
    full = ctx.tfm(s, s, fmc, R.FS, t0=R.T0)
    assert np.array_equal(full, ctx.tfm(s, s, fmc, R.FS, t0=R.T0))
    assert np.array_equal(ctx.tfm(s, s, fmc, R.FS, t0=R.T0, window=R.WINDOW), _sub(full, R.WINDOW))
    assert np.array_equal(ctx.tfm(s, s, fmc, R.FS, t0=R.T0, window=R.WINDOW_STEP3, step=3),
                          _sub(full, R.WINDOW_STEP3, 3))
    small = (34, 66, 2, 3)
    assert np.array_equal(ctx.tfm(s, s, fmc, R.FS, t0=R.T0, window=small), _sub(full, small))


def test_slots_untouched(ctx):
    T, fmc, _, _ = _case(7, 2)
    s = _put(ctx, T)
    before = [ctx.get_field(k, 1) for k in s]
    ctx.tfm(s, s, fmc, R.FS, t0=R.T0)
    assert ctx.get_option("tfm_kernel_ms") > 0 and ctx.get_option("tfm_upload_ms") > 0
    for k in s:
        assert np.array_equal(ctx.get_field(k, 1), before[k]) and np.array_equal(before[k], T[k])


def _raw(ctx, subgrid, tx, rx, fmc, nt, ncomp, t0, fs, w, win, step, image):
    """alifmm_tfm as declared, for the arguments the Python layer cannot express."""
    import _alifmm

    p = lambda a: None if a is None else a.ctypes.data
    rc = _alifmm.lib().alifmm_tfm(ctx._h, subgrid, len(tx) if tx is not None else 1, p(tx),
                                  len(rx) if rx is not None else 1, p(rx), p(fmc), nt, ncomp, t0, fs, p(w), *win, step,
                                  p(image))
    ctx._chk(rc, "tfm")


def test_errors(ctx, envelope):
    import _alifmm

    E = _alifmm.AlifmmError
    T, fmc, ref, mag = _case(7, 2)
    s = _put(ctx, T)
    ctx.put_field(7, 3, np.zeros((109, 208)))
    kw = dict(t0=R.T0)
    # no model
    bare = _alifmm.Context(0)
    with pytest.raises(E, match="no model"):
        bare.tfm([0], [0], fmc[:1, :1], R.FS)
    bare.close()
    bad = [
        lambda: ctx.tfm([0, 999], s, fmc[:2], R.FS, **kw),              # empty slot
        lambda: ctx.tfm(s, [-1] + s[1:], fmc, R.FS, **kw),
        lambda: ctx.tfm(s, s[:6] + [7], fmc, R.FS, **kw),               # mixed subgrids and shapes
        lambda: ctx.tfm(s, s, fmc, R.FS, subgrid=3, **kw),              # not the fields' subgrid
        lambda: ctx.tfm([], s, fmc[:0], R.FS, **kw),                    # ntx < 1
        lambda: ctx.tfm(s, [], fmc[:, :0], R.FS, **kw),                 # nrx < 1
        lambda: ctx.tfm(s, s, fmc[:, :, :1], R.FS, **kw),               # nt < 2
        lambda: ctx.tfm(s, s, fmc, 0.0, **kw),                          # fs
        lambda: ctx.tfm(s, s, fmc, -R.FS, **kw),
        lambda: ctx.tfm(s, s, fmc, math.nan, **kw),
        lambda: ctx.tfm(s, s, fmc, math.inf, **kw),
        lambda: ctx.tfm(s, s, fmc, R.FS, t0=math.nan),                  # t0
        lambda: ctx.tfm(s, s, fmc, R.FS, t0=-math.inf),
        lambda: ctx.tfm(s, s, fmc, R.FS, step=0, **kw),                 # step, niz, nix
        lambda: ctx.tfm(s, s, fmc, R.FS, step=0, window=(0, 0, 1, 1), **kw),
        lambda: ctx.tfm(s, s, fmc, R.FS, window=(0, 0, 0, 5), **kw),
        lambda: ctx.tfm(s, s, fmc, R.FS, window=(0, 0, 5, 0), **kw),
        lambda: ctx.tfm(s, s, fmc, R.FS, window=(0, 0, R.NZ + 1, R.NX), **kw),   # outside the field
        lambda: ctx.tfm(s, s, fmc, R.FS, window=(0, 0, R.NZ, R.NX + 1), **kw),
        lambda: ctx.tfm(s, s, fmc, R.FS, window=(-1, 0, 5, 5), **kw),
        lambda: ctx.tfm(s, s, fmc, R.FS, window=(0, -1, 5, 5), **kw),
        lambda: ctx.tfm(s, s, fmc, R.FS, window=(1, 2, 13, 23), step=3, **kw),
        lambda: ctx.tfm(s, s, fmc, R.FS, window=(5, 5, 2, 2), step=2 ** 30, **kw),
    ]
    # the arguments only the C-ABI can express: ncomp, null pointers
    si = np.asarray(s, dtype=np.int32)
    d = R.as_samples(fmc)
    out = np.empty(FULL[2:] + (2,))
    bad += [
        lambda: _raw(ctx, 1, si, si, d, R.NT, 3, R.T0, R.FS, None, FULL, 1, out),
        lambda: _raw(ctx, 1, si, si, d, R.NT, 0, R.T0, R.FS, None, FULL, 1, out),
        lambda: _raw(ctx, 1, None, si, d, R.NT, 2, R.T0, R.FS, None, FULL, 1, out),
        lambda: _raw(ctx, 1, si, None, d, R.NT, 2, R.T0, R.FS, None, FULL, 1, out),
        lambda: _raw(ctx, 1, si, si, None, R.NT, 2, R.T0, R.FS, None, FULL, 1, out),
        lambda: _raw(ctx, 1, si, si, d, R.NT, 2, R.T0, R.FS, None, FULL, 1, None),
        # a window whose extent passes 2^31 (validated in 64-bit, before anything is allocated)
        lambda: _raw(ctx, 1, si, si, d, R.NT, 2, R.T0, R.FS, None, (5, 5, 2 ** 31 - 1, 2), 2 ** 31 - 1, out),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(E, match="rc=-2|tfm: step"):
            call()
            pytest.fail("rejected input %d was accepted" % k)
    # the context is still usable: the valid call passes as in test_element_counts
    _raw(ctx, 1, si, si, d, R.NT, 2, R.T0, R.FS, None, FULL, 1, out)
    _check(envelope, "after_errors_raw", out.view(np.complex128)[..., 0], ref, 49, mag)
    _check(envelope, "after_errors", ctx.tfm(s, s, fmc, R.FS, **kw), ref, 49, mag)


def test_end_to_end_through_the_dropin(envelope):
    """ALI_FMM.tfm on computed fields: a point scatterer synthesised from the fields update()
    returns focuses at its node, and the image is the reference's on those fields."""
    import Anis_TTF_rays as A

    n, dnx, fs = 61, 1e-3, R.FS
    veln = W.voronoi_small(n, seed=7)
    velpn = np.zeros((n, n), dtype=np.int64)
    vm = np.ones((n, n))
    sd = W.stif_field(n, n)
    xs = np.arange(6, 56, 7)
    assert len(xs) == 8
    M = A.ALI_FMM(veln, velpn, vm, dnx * xs.astype(float), np.zeros(8), stif_den=sd, dnx=dnx)
    F = M.update(veln, velpn, vm, sd)
    q = (40, 23)
    tq = F[:, q[0], q[1]]
    nt = math.ceil(2 * F.max() * fs) + 2
    fmc = R.scatterer_data(tq, tq, fs, nt)
    img = M.tfm(fmc, fs)
    ref, mag, cnt = R.tfm_ref(F, F, fmc, fs)
    assert cnt["inside"] == 64 * n * n
    _check(envelope, "dropin", img, ref, 64, mag)
    a = np.abs(img)
    peak = np.unravel_index(a.argmax(), a.shape)
    print("peak %.1f at %s" % (a[peak], peak))
    assert abs(peak[0] - q[0]) <= 1 and abs(peak[1] - q[1]) <= 1 and a[peak] >= 0.7 * 64
    tx = [0, 2, 4, 6]
    sub = M.tfm(fmc[tx], fs, tx=tx)
    rsub, msub, _ = R.tfm_ref(F[tx], F, fmc[tx], fs)
    _check(envelope, "dropin_tx_subset", sub, rsub, 32, msub)
