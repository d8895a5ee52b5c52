"""GPU tests of the coherence-weighted TFM over resident fields (include/alifmm.h alifmm_tfm_coh,
csrc/tfm_coh.hip) against the numpy restatement of its contract (tests/tfm_coh_ref.py), on the
synthetic 37 x 70 case of tests/tfm_ref.py: the fields are uploaded with put_field, so the kernel
runs on exactly known delays.

The bars are derived, not measured.  No operation is contracted and every one (sqrt and / included)
is correctly rounded on both sides, so each term is the same float64 number in numpy and on the
device; only the order of the sums differs.
  image   np.array_equal to ctx.tfm of the same call (the same statements in the same order), and
          with it within tfm_ref.bound of the reference.
  n, b    sums of small integers: equal to the reference, for every tfm_chunk.
  q       a sum of npairs non-negative terms in any order is within (npairs - 1) 2^-53 of the exact
          sum, relatively: |q - q_ref| <= 2 (npairs + 4) 2^-53 q_ref.
  ph_c    each term has magnitude <= 1, so sum |term| <= n: |ph_c - ph_c,ref| <= 2 (npairs + 4) 2^-53 n.
  factor  bit-equal to the contract's formula evaluated in numpy on the call's own image and sums.
          Against the reference's sums (recorded, and asserted too): the bars above propagated
          through the formula, tfm_coh_ref.factor_bar, with |sqrt(y1) - sqrt(y2)| <= sqrt(|y1 - y2|).
Where no term counts, image, factor and sums are exactly 0.  The worst ratio of each case goes to
the session's envelope under tfm_coh/... ."""
import math

import numpy as np
import pytest

import tfm_coh_ref as C
import tfm_ref as R
import workloads as W

pytestmark = pytest.mark.gpu

FULL = R.full_window((R.NZ, R.NX))
KINDS = ("cf", "scf", "pcf")


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    c.set_model(np.zeros((R.NZ, R.NX)), np.ones((R.NZ, R.NX), dtype=np.int64), np.full((R.NZ, R.NX), R.SPEED), None,
                W.default_table(), W.default_table(), R.DNX)
    yield c
    c.close()


_cache = {}


def _case(n, ncomp, kind):
    """Fields, data and the full-window reference of n elements (computed once, never modified)."""
    key = (n, ncomp, kind)
    if key not in _cache:
        T = R.fields(R.element_x(n))
        fmc = R.data(n, n, ncomp=ncomp)
        ref = C.tfm_coh_ref(T, T, fmc, R.FS, kind, R.T0)
        for a in (T, fmc) + ref:
            a.setflags(write=False)
        _cache[key] = (T, fmc, ref)
    return _cache[key]


def _put(ctx, T, first=0, subgrid=1):
    for k, f in enumerate(T):
        ctx.put_field(first + k, subgrid, f)
    return list(range(first, first + len(T)))


def _sub(a, window, step=1):
    z, x, nz, nx = window
    return a[z:z + step * nz:step, x:x + step * nx:step]


def _check(envelope, name, kind, got, ref, npairs, plain=None):
    """The module's bars on one call's (image, factor, sums) against the reference's."""
    img, fac, sums = got
    rimg, _, rsums, mag = ref
    assert img.shape == rimg.shape and img.dtype == rimg.dtype and fac.shape == rimg.shape and sums.shape == rsums.shape
    if plain is not None:
        assert np.array_equal(img, plain)
    r = {"image": R.worst_ratio(img, rimg, npairs, mag), "sums": C.sums_ratio(kind, sums, rsums, npairs),
         "factor": C.factor_ratio(kind, fac, rimg, rsums, npairs, mag)}
    for k, v in r.items():
        envelope["tfm_coh/%s_%s" % (name, k)] = v
    print("tfm_coh/%s: worst error / bar: image %.3g, sums %.3g, factor (against the reference's sums) %.3g"
          % (name, r["image"], r["sums"], r["factor"]))
    assert max(r.values()) <= 1.0, (name, r)
    assert np.array_equal(fac, C.factor_of(kind, img, sums))
    none = rsums[..., 0] == 0
    assert np.all(img[none] == 0) and not fac[none].any() and not sums[none].any()


@pytest.mark.parametrize("ncomp,kind", [(2, "cf"), (2, "scf"), (2, "pcf"), (1, "cf"), (1, "scf")])
@pytest.mark.parametrize("n", [1, 7, 65])
def test_element_counts_and_kinds(ctx, envelope, n, ncomp, kind):
    """65 crosses the receiver chunk with a partial last chunk, 1 puts every pixel at |m| = 1, the
    ill-conditioned end of 1 - sqrt(1 - m²); the full window (tail tiles in x and z) and a window
    aligned to no tile."""
    T, fmc, ref = _case(n, ncomp, kind)
    s = _put(ctx, T)
    for name, win in (("full", None), ("window", R.WINDOW)):
        got = ctx.tfm_coh(s, s, fmc, R.FS, kind=kind, t0=R.T0, window=win, sums=True)
        plain = ctx.tfm(s, s, fmc, R.FS, t0=R.T0, window=win)
        sub = ref if win is None else tuple(_sub(a, win) for a in ref)
        _check(envelope, "n%d_c%d_%s_%s" % (n, ncomp, kind, name), kind, got, sub, n * n, plain)
        two = ctx.tfm_coh(s, s, fmc, R.FS, kind=kind, t0=R.T0, window=win)  # without the sums
        assert len(two) == 2 and np.array_equal(two[0], got[0]) and np.array_equal(two[1], got[1])
    if n == 1:  # one term: CF and SCF are exactly 1 (the last call, the window)
        one = sub[2][..., 0] == 1
        assert one.any() and sub[2][..., 0].max() == 1 and (kind == "pcf" or np.all(got[1][one] == 1))


def test_weights_and_nonfinite_fields(ctx, envelope):
    """Weights with zeros and negative values; then NaN, +inf, -1.0 and 1e300 patches in the fields
    (test_gpu_tfm.py::test_nonfinite_fields): every pair touching them adds nothing to any sum, and
    where every field is patched n == 0 and image, factor and sums are exactly 0."""
    T0, fmc, _ = _case(7, 2, "cf")
    s = _put(ctx, T0)
    rng = np.random.default_rng(8)
    w = rng.standard_normal((7, 7)).astype(np.float32)
    w[rng.random((7, 7)) < 0.3] = 0
    assert 0 < (w == 0).sum() < 49 and (w < 0).any()
    for kind in KINDS:
        got = ctx.tfm_coh(s, s, fmc, R.FS, kind=kind, t0=R.T0, weights=w, sums=True)
        _check(envelope, "weights_" + kind, kind, got, C.tfm_coh_ref(T0, T0, fmc, R.FS, kind, R.T0, w), 49,
               ctx.tfm(s, s, fmc, R.FS, t0=R.T0, weights=w))
        zero = ctx.tfm_coh(s, s, fmc, R.FS, kind=kind, t0=R.T0, weights=np.zeros((7, 7)), sums=True)
        assert not zero[0].real.any() and not zero[0].imag.any() and not zero[1].any() and not zero[2].any()
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
    for kind in KINDS:
        for name, wt in (("nonfinite", None), ("nonfinite_w", w)):
            img, fac, sums = got = ctx.tfm_coh(s, s, fmc, R.FS, kind=kind, t0=R.T0, weights=wt, sums=True)
            ref = C.tfm_coh_ref(T, T, fmc, R.FS, kind, R.T0, wt)
            assert not ref[2][12:16, 30:41, 0].any() and ref[2][5:8, 10:14, 0].all()
            assert np.all(img[12:16, 30:41] == 0) and not fac[12:16, 30:41].any() and not sums[12:16, 30:41].any()
            assert np.isfinite(img.real).all() and np.isfinite(img.imag).all() and np.isfinite(fac).all()
            assert np.isfinite(sums).all()
            _check(envelope, "%s_%s" % (name, kind), kind, got, ref, 49, ctx.tfm(s, s, fmc, R.FS, t0=R.T0, weights=wt))


def test_chunk_option_and_determinism(ctx, envelope):
    """Every value of option tfm_chunk: the image is ctx.tfm's at that chunk, n and b do not
    depend on it, q and ph stay within their bars.  The same call twice gives the same bits, and a
    pixel has the same bits through every window and step.  Subgrid 3 as in test_gpu_tfm.py."""
    default = int(ctx.get_option("tfm_chunk"))
    for kind in KINDS:
        T, fmc, ref = _case(65, 2, kind)
        s = _put(ctx, T)
        try:
            for c in (4, 8, 16, 32):
                ctx.set_option("tfm_chunk", c)
                got = ctx.tfm_coh(s, s, fmc, R.FS, kind=kind, t0=R.T0, sums=True)
                _check(envelope, "chunk%d_%s" % (c, kind), kind, got, ref, 65 * 65, ctx.tfm(s, s, fmc, R.FS, t0=R.T0))
                assert np.array_equal(got[2][..., 0], ref[2][..., 0])
                assert kind != "scf" or np.array_equal(got[2], ref[2])
        finally:
            ctx.set_option("tfm_chunk", default)
        full = ctx.tfm_coh(s, s, fmc, R.FS, kind=kind, t0=R.T0, sums=True)
        again = ctx.tfm_coh(s, s, fmc, R.FS, kind=kind, t0=R.T0, sums=True)
        win = ctx.tfm_coh(s, s, fmc, R.FS, kind=kind, t0=R.T0, window=R.WINDOW, sums=True)
        st3 = ctx.tfm_coh(s, s, fmc, R.FS, kind=kind, t0=R.T0, window=R.WINDOW_STEP3, step=3, sums=True)
        for k in range(3):
            assert np.array_equal(full[k], again[k], equal_nan=True)
            assert np.array_equal(win[k], _sub(full[k], R.WINDOW))
            assert np.array_equal(st3[k], _sub(full[k], R.WINDOW_STEP3, 3))
    # subgrid 3: fine shape 109 x 208
    assert ctx.field_shape(3) == (109, 208)
    T, fmc, _ = _case(7, 2, "pcf")
    T3 = R.fields(3 * R.element_x(7), nz=109, nx=208, dnx=R.DNX / 3)
    s3 = _put(ctx, T3, first=65, subgrid=3)
    got = ctx.tfm_coh(s3, s3, fmc, R.FS, kind="pcf", t0=R.T0, subgrid=3, sums=True)
    _check(envelope, "subgrid3", "pcf", got, C.tfm_coh_ref(T3, T3, fmc, R.FS, "pcf", R.T0), 49,
           ctx.tfm(s3, s3, fmc, R.FS, t0=R.T0, subgrid=3))
    w3 = (5, 7, 33, 65)
    win = ctx.tfm_coh(s3, s3, fmc, R.FS, kind="pcf", t0=R.T0, subgrid=3, window=w3, step=3, sums=True)
    for k in range(3):
        assert np.array_equal(win[k], _sub(got[k], w3, 3))


def _raw(ctx, subgrid, tx, rx, fmc, nt, ncomp, t0, fs, w, win, step, kind, image, factor, sums):
    """alifmm_tfm_coh as declared, for the arguments the Python layer cannot express."""
    import _alifmm

    p = lambda a: None if a is None else a.ctypes.data
    rc = _alifmm.lib().alifmm_tfm_coh(ctx._h, subgrid, len(tx) if tx is not None else 1, p(tx),
                                      len(rx) if rx is not None else 1, p(rx), p(fmc), nt, ncomp, t0, fs, p(w), *win, step,
                                      kind, p(image), p(factor), p(sums))
    ctx._chk(rc, "tfm_coh")


def test_errors(ctx, envelope):
    import _alifmm

    E = _alifmm.AlifmmError
    T, fmc, ref = _case(7, 2, "cf")
    s = _put(ctx, T)
    ctx.put_field(7, 3, np.zeros((109, 208)))
    before = [ctx.get_field(k, 1) for k in s]
    kw = dict(t0=R.T0)
    bare = _alifmm.Context(0)
    with pytest.raises(E, match="no model"):
        bare.tfm_coh([0], [0], fmc[:1, :1], R.FS)
    bare.close()
    with pytest.raises(ValueError):
        ctx.tfm_coh(s, s, fmc, R.FS, kind="das", **kw)
    bad = [
        lambda: ctx.tfm_coh([0, 999], s, fmc[:2], R.FS, **kw),              # empty slot
        lambda: ctx.tfm_coh(s, [-1] + s[1:], fmc, R.FS, **kw),
        lambda: ctx.tfm_coh(s, s[:6] + [7], fmc, R.FS, **kw),               # mixed subgrids and shapes
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, subgrid=3, **kw),              # not the fields' subgrid
        lambda: ctx.tfm_coh([], s, fmc[:0], R.FS, **kw),                    # ntx < 1
        lambda: ctx.tfm_coh(s, [], fmc[:, :0], R.FS, **kw),                 # nrx < 1
        lambda: ctx.tfm_coh(s, s, fmc[:, :, :1], R.FS, **kw),               # nt < 2
        lambda: ctx.tfm_coh(s, s, fmc, 0.0, **kw),                          # fs
        lambda: ctx.tfm_coh(s, s, fmc, -R.FS, **kw),
        lambda: ctx.tfm_coh(s, s, fmc, math.nan, **kw),
        lambda: ctx.tfm_coh(s, s, fmc, math.inf, **kw),
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, t0=math.nan),                  # t0
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, t0=-math.inf),
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, step=0, **kw),                 # step, niz, nix
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, step=0, window=(0, 0, 1, 1), **kw),
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, window=(0, 0, 0, 5), **kw),
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, window=(0, 0, 5, 0), **kw),
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, window=(0, 0, R.NZ + 1, R.NX), **kw),   # outside the field
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, window=(0, 0, R.NZ, R.NX + 1), **kw),
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, window=(-1, 0, 5, 5), **kw),
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, window=(0, -1, 5, 5), **kw),
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, window=(1, 2, 13, 23), step=3, **kw),
        lambda: ctx.tfm_coh(s, s, fmc, R.FS, window=(5, 5, 2, 2), step=2 ** 30, **kw),
        lambda: ctx.tfm_coh(s, s, fmc.real, R.FS, kind="pcf", **kw),        # PCF of real data
    ]
    # the arguments only the C-ABI can express: ncomp, kind, null pointers; nothing is written
    si = np.asarray(s, dtype=np.int32)
    d = R.as_samples(fmc)
    img, fac, sums = np.full(FULL[2:] + (2,), 7.5), np.full(FULL[2:], 7.5), np.full(FULL[2:] + (3,), 7.5)
    a = (R.T0, R.FS, None, FULL, 1)
    bad += [
        lambda: _raw(ctx, 1, si, si, d, R.NT, 3, *a, 1, img, fac, sums),
        lambda: _raw(ctx, 1, si, si, d, R.NT, 0, *a, 1, img, fac, sums),
        lambda: _raw(ctx, 1, si, si, d, R.NT, 2, *a, 0, img, fac, sums),     # kind
        lambda: _raw(ctx, 1, si, si, d, R.NT, 2, *a, 4, img, fac, sums),
        lambda: _raw(ctx, 1, si, si, d, R.NT, 2, *a, -1, img, fac, sums),
        lambda: _raw(ctx, 1, si, si, d, 2 * R.NT, 1, *a, 3, img, fac, sums),  # kind 3 with ncomp 1
        lambda: _raw(ctx, 1, None, si, d, R.NT, 2, *a, 1, img, fac, sums),
        lambda: _raw(ctx, 1, si, None, d, R.NT, 2, *a, 1, img, fac, sums),
        lambda: _raw(ctx, 1, si, si, None, R.NT, 2, *a, 1, img, fac, sums),
        lambda: _raw(ctx, 1, si, si, d, R.NT, 2, *a, 1, None, fac, sums),
        lambda: _raw(ctx, 1, si, si, d, R.NT, 2, *a, 1, img, None, sums),
        lambda: _raw(ctx, 1, si, si, d, R.NT, 2, *a, 1, img, None, None),
        # a window whose extent passes 2^31 (validated in 64-bit, before anything is allocated)
        lambda: _raw(ctx, 1, si, si, d, R.NT, 2, R.T0, R.FS, None, (5, 5, 2 ** 31 - 1, 2), 2 ** 31 - 1, 1, img, fac, sums),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(E, match="rc=-2|tfm_coh: step"):
            call()
            pytest.fail("rejected input %d was accepted" % k)
    assert np.all(img == 7.5) and np.all(fac == 7.5) and np.all(sums == 7.5)
    # the context is still usable: the valid call passes as in test_element_counts_and_kinds
    _raw(ctx, 1, si, si, d, R.NT, 2, *a, 1, img, fac, sums)
    _check(envelope, "after_errors_raw", "cf", (img.view(np.complex128)[..., 0], fac, sums), ref, 49)
    _check(envelope, "after_errors", "cf", ctx.tfm_coh(s, s, fmc, R.FS, sums=True, **kw), ref, 49)
    assert ctx.get_option("tfm_coh_kernel_ms") > 0 and ctx.get_option("tfm_coh_upload_ms") > 0
    for k in s:  # the slots are untouched
        assert np.array_equal(ctx.get_field(k, 1), before[k]) and np.array_equal(before[k], T[k])


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_demonstration(ctx, envelope, seed):
    """A point scatterer in complex Gaussian noise, 8 elements (the inputs that
    test_tfm_coh_ref.py::test_demonstration_case_meets_its_conditions checks in the reference): for
    every kind the weighted image peaks at the scatterer, F >= 0.5 there and <= 0.2 outside the
    5 x 5 block around it, and the peak-to-background ratio gains at least 4 x over the plain image."""
    T, fmc = C.demo_case(seed)
    s = _put(ctx, T)
    for kind in KINDS:
        got = ctx.tfm_coh(s, s, fmc, R.FS, kind=kind, sums=True)
        _check(envelope, "demo%d_%s" % (seed, kind), kind, got, C.tfm_coh_ref(T, T, fmc, R.FS, kind), 64,
               ctx.tfm(s, s, fmc, R.FS))
        f_in, f_out, gain = C.demo_check(got[0], got[1])
        print("seed %d %s: F %.3f at the scatterer, <= %.3f elsewhere, ratio gain %.1f x" % (seed, kind, f_in, f_out, gain))


def test_end_to_end_through_the_dropin(envelope):
    """ALI_FMM.tfm_coherence on computed fields (the 61² Voronoi model of test_gpu_tfm.py): the
    factor is the reference's on the fields update() returns, the weighted image is image * factor
    within what the two bars allow (|I F - I_ref F_ref| <= |I - I_ref| F_ref + (|I_ref| + |I - I_ref|)
    |F - F_ref|, and 4 * 2^-53 |I_ref| F_ref for the product's roundings), and power 0 gives tfm()'s bits."""
    import Anis_TTF_rays as A

    n, dnx, fs = 61, 1e-3, R.FS
    veln = W.voronoi_small(n, seed=7)
    velpn = np.zeros((n, n), dtype=np.int64)
    vm = np.ones((n, n))
    sd = W.stif_field(n, n)
    xs = np.arange(6, 56, 7)
    M = A.ALI_FMM(veln, velpn, vm, dnx * xs.astype(float), np.zeros(8), stif_den=sd, dnx=dnx)
    F = M.update(veln, velpn, vm, sd)
    q = (40, 23)
    tq = F[:, q[0], q[1]]
    nt = math.ceil(2 * F.max() * fs) + 2
    fmc = R.scatterer_data(tq, tq, fs, nt)
    plain = M.tfm(fmc, fs)
    for kind in KINDS:
        rimg, rfac, rsums, mag = C.tfm_coh_ref(F, F, fmc, fs, kind)
        assert np.all(rsums[..., 0] == 64)
        img, fac = M.tfm_coherence(fmc, fs, kind=kind)
        assert img.shape == rimg.shape and img.dtype == rimg.dtype and fac.shape == rfac.shape
        d, fb = R.bound(64, mag), C.factor_bar(kind, rimg, rsums, 64, mag)
        assert np.all(np.abs(fac - rfac) <= fb)
        e = img - rimg * rfac
        err = np.maximum(np.abs(e.real), np.abs(e.imag))
        top = np.maximum(np.abs(rimg.real), np.abs(rimg.imag))
        r = float((err / (d * rfac + (top + d) * fb + 4 * C.U * top * rfac + 1e-300)).max())
        envelope["tfm_coh/dropin_" + kind] = r
        print("tfm_coh/dropin_%s: worst error / bar of the weighted image %.3g" % (kind, r))
        assert r <= 1.0
        a = np.abs(img)
        peak = np.unravel_index(a.argmax(), a.shape)
        assert abs(peak[0] - q[0]) <= 1 and abs(peak[1] - q[1]) <= 1 and fac[peak] >= 0.5
        zero, f0 = M.tfm_coherence(fmc, fs, kind=kind, power=0.0)
        assert np.array_equal(zero, plain) and np.array_equal(f0, fac)
    tx = [0, 2, 4, 6]
    img, fac = M.tfm_coherence(fmc[tx], fs, kind="pcf", power=2.0, tx=tx)
    rimg, rfac, rsums, mag = C.tfm_coh_ref(F[tx], F, fmc[tx], fs, "pcf")
    assert np.all(np.abs(fac - rfac) <= C.factor_bar("pcf", rimg, rsums, 32, mag))
    sub = M.tfm(fmc[tx], fs, tx=tx)
    assert np.array_equal(img, sub * fac ** 2.0)
