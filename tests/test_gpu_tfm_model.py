"""GPU tests of FMC modelling over resident fields (include/alifmm.h alifmm_tfm_model,
csrc/tfm_model.hip), the transpose of the TFM sum, against the numpy restatement of its contract
(tests/tfm_model_ref.py).  The fields are uploaded with put_field after set_model of the isotropic
37 x 70 model of test_gpu_tfm.py, so the kernel runs on exactly known delays.

The bar of every data comparison, per sample and component: |d - d_ref| <= 2 (n + 4) 2^-53 A,
n the contributions to the sample and A the sum of their |w| max_c |refl_c| (derived in
tfm_model_ref.bound); a sample without contributions must be exactly 0.  The bar of the adjoint
identity is tfm_model_ref.adjoint_bar's.  The order of the device's sums is not fixed, so no test
asserts bit equality between two runs.  The worst measured ratio of each case goes to the
session's envelope under tfm_model/... ."""
import math

import numpy as np
import pytest

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


_cache = {}


def _case(n, ncomp, window=FULL, nt=R.NT):
    """Fields, map and reference of n elements on a window (computed once, never modified)."""
    key = (n, ncomp, window, nt)
    if key not in _cache:
        T = R.fields(R.element_x(n))
        x = M.noise_map(window[2:], ncomp)
        ref, A, cn, cnt = M.model_ref(T, T, x, nt, R.FS, R.T0, None, window)
        assert cnt["inside"] > 0
        for a in (T, x, ref, A, cn):
            a.setflags(write=False)
        _cache[key] = (T, x, ref, A, cn)
    return _cache[key]


def _put(ctx, T, first=0, subgrid=1):
    for k, f in enumerate(T):
        ctx.put_field(first + k, subgrid, f)
    return list(range(first, first + len(T)))


def _check(envelope, name, d, ref, cn, A):
    assert d.shape == ref.shape and d.dtype == ref.dtype
    r = M.worst_ratio(d, ref, cn, A)
    envelope["tfm_model/" + name] = r
    print("tfm_model/%s: worst |d - d_ref| / bound = %.3g" % (name, r))
    assert r <= 1.0, (name, r)
    assert not d[cn == 0].real.any() and not d[cn == 0].imag.any()


@pytest.mark.parametrize("n,ncomp", [(1, 2), (7, 2), (65, 2), (7, 1)])
def test_element_counts(ctx, envelope, n, ncomp):
    """1 and 7 end in a half-empty receiver group, 65 has many groups and one slab; the full window
    and a window aligned to nothing, default knobs."""
    for name, win in (("full", FULL), ("window", R.WINDOW)):
        T, x, ref, A, cn = _case(n, ncomp, win)
        s = _put(ctx, T)
        d = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0, window=None if win == FULL else win)
        _check(envelope, "n%d_c%d_%s" % (n, ncomp, name), d, ref, cn, A)
        assert ctx.get_option("tfm_model_tile_used") == R.NT
        assert ctx.get_option("tfm_model_tile") == 0 and ctx.get_option("tfm_model_slabs") == 0


def test_tiles(ctx, envelope):
    """tfm_model_tile 64 at nt = 480 (7.5 tiles) and nt = 65 (a last tile of one sample), nt = 2, and
    the largest tile (two complex traces of 4096 samples, 128 KiB of LDS): the bar of the automatic
    tile."""
    T = R.fields(R.element_x(7))
    s = _put(ctx, T)
    try:
        for nt in (R.NT, 65):
            _, x, ref, A, cn = _case(7, 2, R.WINDOW, nt)
            assert M.tile_edge_fraction(T, T, x, nt, R.FS, R.T0, None, R.WINDOW, 1, 64) >= 0.01
            ctx.set_option("tfm_model_tile", 64)
            d = ctx.tfm_model(s, s, x, R.FS, nt, t0=R.T0, window=R.WINDOW)
            assert ctx.get_option("tfm_model_tile_used") == 64 and ctx.get_option("tfm_model_tile") == 64
            _check(envelope, "tile64_nt%d" % nt, d, ref, cn, A)
            ctx.set_option("tfm_model_tile", 0)
            d = ctx.tfm_model(s, s, x, R.FS, nt, t0=R.T0, window=R.WINDOW)
            assert ctx.get_option("tfm_model_tile_used") == nt and ctx.get_option("tfm_model_tile") == 0
            _check(envelope, "tile0_nt%d" % nt, d, ref, cn, A)
        # nt = 2: only u in [0, 1) is in range
        x = _case(7, 2)[1]
        fs, t0 = 1.2e5, 2e-6
        ref, A, cn, cnt = M.model_ref(T, T, x, 2, fs, t0)
        assert cnt["inside"] > 0 and cnt["below"] > 0 and cnt["above"] > 0
        for tile, used in ((0, 2), (64, 2), (1, 1)):
            ctx.set_option("tfm_model_tile", tile)
            d = ctx.tfm_model(s, s, x, fs, 2, t0=t0)
            assert ctx.get_option("tfm_model_tile_used") == used
            _check(envelope, "nt2_tile%d" % tile, d, ref, cn, A)
        # nt = 5000 complex: the automatic tile is the 4096 samples that fit, in two passes
        ctx.set_option("tfm_model_tile", 0)
        fs = 5000 / 480 * R.FS
        ref, A, cn, cnt = M.model_ref(T[:3], T[:3], x, 5000, fs, R.T0)
        assert cn[:, :, 4096:].any() and cn[:, :, :4096].any()
        d = ctx.tfm_model(s[:3], s[:3], x, fs, 5000, t0=R.T0)
        assert ctx.get_option("tfm_model_tile_used") == 4096
        _check(envelope, "nt5000", d, ref, cn, A)
    finally:
        ctx.set_option("tfm_model_tile", 0)
    with pytest.raises(Exception):
        ctx.set_option("tfm_model_tile", -1)
    with pytest.raises(Exception):
        ctx.set_option("tfm_model_tile", 64.5)
    assert ctx.get_option("tfm_model_tile") == 0


def test_slabs(ctx, envelope):
    """tfm_model_slabs 1 (plain stores), 3, 8 and 64 (more than the 37 pixel rows; atomic flush into
    the zeroed output), and automatic: the same bar.  A one-pixel map cuts the slabs to 1."""
    T, x, ref, A, cn = _case(7, 2)
    s = _put(ctx, T)
    try:
        for k in (1, 3, 8, 64):
            ctx.set_option("tfm_model_slabs", k)
            d = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0)
            assert ctx.get_option("tfm_model_slabs_used") == k and ctx.get_option("tfm_model_slabs") == k
            _check(envelope, "slabs%d" % k, d, ref, cn, A)
        one = np.zeros(FULL[2:], dtype=np.complex128)
        one[20, 33] = 1 - 2j
        ctx.tfm_model(s, s, one, R.FS, R.NT, t0=R.T0)
        assert ctx.get_option("tfm_model_slabs_used") == 1
        ctx.set_option("tfm_model_slabs", 0)
        d = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0)
        assert 1 <= ctx.get_option("tfm_model_slabs_used") <= 64 and ctx.get_option("tfm_model_slabs") == 0
        _check(envelope, "slabs_auto", d, ref, cn, A)
    finally:
        ctx.set_option("tfm_model_slabs", 0)
    for bad in (-1, 65, 2.5):
        with pytest.raises(Exception):
            ctx.set_option("tfm_model_slabs", bad)
    with pytest.raises(Exception):
        ctx.set_option("tfm_model_slabs_used", 1)
    assert ctx.get_option("tfm_model_slabs") == 0


def test_receivers_and_combine(ctx, envelope):
    """Every value of tfm_model_rx (receivers per workgroup; 7 receivers leave a partly empty last
    group for 2 and 4) without, with the default and with unconditional wave-level pre-combination (tfm_model_combine 0, 12, 64), on the
    half-zero map and on a dense one, whose runs of lanes sharing a sample are long and cross the
    rows of 16 lanes and the wave's halves; complex and real.  Another summation order, the same bar."""
    T = R.fields(R.element_x(7))
    s = _put(ctx, T)
    assert ctx.get_option("tfm_model_rx") == 2 and ctx.get_option("tfm_model_combine") == 12
    maps = [("half", 2, _case(7, 2)[1]), ("dense", 2, M.noise_map(FULL[2:], 2, seed=31, keep=1.0)),
            ("dense", 1, M.noise_map(FULL[2:], 1, seed=32, keep=1.0))]
    try:
        for name, nc, x in maps:
            ref, A, cn, _ = M.model_ref(T, T, x, R.NT, R.FS, R.T0)
            for rx in (1, 2, 4):
                for comb in (0, 12, 64):
                    ctx.set_option("tfm_model_rx", rx)
                    ctx.set_option("tfm_model_combine", comb)
                    d = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0)
                    _check(envelope, "%s_c%d_rx%d_combine%d" % (name, nc, rx, comb), d, ref, cn, A)
        # a slow field: whole waves share one sample (delays of 0.002 samples per pixel)
        flat = np.stack([(100.3 + 0.001 * np.arange(R.NZ * R.NX).reshape(R.NZ, R.NX) + 7 * e) / R.FS for e in range(7)])
        sf = _put(ctx, flat)
        x = maps[1][2]
        ref, A, cn, _ = M.model_ref(flat, flat, x, R.NT, R.FS, 0.0)
        assert cn.max() >= 500
        for comb in (0, 12, 64):
            ctx.set_option("tfm_model_rx", 2)
            ctx.set_option("tfm_model_combine", comb)
            d = ctx.tfm_model(sf, sf, x, R.FS, R.NT)
            _check(envelope, "flat_combine%d" % comb, d, ref, cn, A)
    finally:
        ctx.set_option("tfm_model_rx", 2)
        ctx.set_option("tfm_model_combine", 12)
    for name, bad in (("tfm_model_rx", 3), ("tfm_model_rx", 0), ("tfm_model_combine", 65), ("tfm_model_combine", -1)):
        with pytest.raises(Exception):
            ctx.set_option(name, bad)


def test_slot_lists(ctx, envelope):
    """ntx 5 against nrx 9; tx reversed with one slot repeated, rx a strided subset, slots not
    starting at 0: a swapped or transposed index shows."""
    T = R.fields(R.element_x(24))
    _put(ctx, T, first=3)
    tx = [3 + e for e in (20, 11, 11, 4, 1)]
    rx = list(range(3 + 2, 3 + 2 + 18, 2))
    x = _case(7, 2)[1]
    d = ctx.tfm_model(tx, rx, x, R.FS, R.NT, t0=R.T0)
    ref, A, cn, _ = M.model_ref(T[[s - 3 for s in tx]], T[[s - 3 for s in rx]], x, R.NT, R.FS, R.T0)
    _check(envelope, "slot_lists", d, ref, cn, A)
    swapped, _, _, _ = M.model_ref(T[[s - 3 for s in rx]][:5], T[[s - 3 for s in tx] + [0] * 4], x, R.NT, R.FS, R.T0)
    e = np.maximum(np.abs((swapped - ref).real), np.abs((swapped - ref).imag))
    assert (e[cn > 0] > 1e6 * M.bound(cn, A)[cn > 0]).any()  # the reference itself tells the lists apart


def test_weights(ctx, envelope):
    T, x, _, _, _ = _case(7, 2)
    s = _put(ctx, T)
    rng = np.random.default_rng(8)
    w = rng.standard_normal((7, 7)).astype(np.float32)
    w[rng.random((7, 7)) < 0.3] = 0
    assert 0 < (w == 0).sum() < 49 and (w < 0).any()
    d = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0, weights=w)
    ref, A, cn, cnt = M.model_ref(T, T, x, R.NT, R.FS, R.T0, w)
    assert cnt["zero_weight"] > 0
    _check(envelope, "weights", d, ref, cn, A)
    assert not d[w == 0].real.any() and not d[w == 0].imag.any()
    zero = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0, weights=np.zeros((7, 7)))
    assert zero.shape == (7, 7, R.NT) and not zero.real.any() and not zero.imag.any()


def test_nonfinite_fields(ctx, envelope):
    """The NaN, +inf, -1.0 and 1e300 patches of test_gpu_tfm.py::test_nonfinite_fields: every pair
    touching them gets nothing from those pixels, the output is finite and within the bar."""
    T0, x, _, _, _ = _case(7, 2)
    T = T0.copy()
    bad = [np.nan, np.inf, -1.0, 1e300]
    T[0, 5:8, 10:14] = np.nan
    T[2, 20:30, 60:70] = -1.0
    T[3, 0:4, 0:70] = 1e300
    T[5, 30:37, 0:9] = np.inf
    for e in range(7):  # every field patched here, by one of the four values
        T[e, 12:16, 30:41] = bad[e % 4]
    assert x[12:16, 30:41].any() and x[5:8, 10:14].any()
    s = _put(ctx, T)
    w = np.ones((7, 7), dtype=np.float32)
    w[0, 3] = 0  # a zero weight on a NaN delay
    for name, wt in (("nonfinite", None), ("nonfinite_w", w)):
        d = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0, weights=wt)
        ref, A, cn, cnt = M.model_ref(T, T, x, R.NT, R.FS, R.T0, wt)
        assert cnt["nonfinite"] > 0 and cnt["below"] > 0 and cnt["above"] > 0
        assert np.isfinite(d.real).all() and np.isfinite(d.imag).all()
        _check(envelope, name, d, ref, cn, A)


def test_exactness(ctx):
    """One non-zero pixel: every pair has two non-zero samples, each with one contribution, and the
    output equals the reference exactly, through plain stores and through the atomic flush.  An
    all-zero map gives +0.0 everywhere."""
    T = R.fields(R.element_x(7))
    s = _put(ctx, T)
    x = np.zeros(FULL[2:], dtype=np.complex128)
    x[20, 33] = 0.7 - 1.3j
    ref, A, cn, cnt = M.model_ref(T, T, x, R.NT, R.FS, R.T0)
    assert cnt["inside"] == 49 and cn.max() == 1
    d = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0)
    assert np.array_equal(d, ref)
    assert (np.count_nonzero(d, axis=2) == 2).all()
    x2 = x.copy()
    x2[3, 60] = -2.5  # two pixels, one per slab: a sample with one contribution is still exactly that value
    ref2, A2, cn2, _ = M.model_ref(T, T, x2, R.NT, R.FS, R.T0)
    try:
        ctx.set_option("tfm_model_slabs", 2)
        d2 = ctx.tfm_model(s, s, x2, R.FS, R.NT, t0=R.T0)
        assert ctx.get_option("tfm_model_slabs_used") == 2
    finally:
        ctx.set_option("tfm_model_slabs", 0)
    assert np.array_equal(d2[cn2 <= 1], ref2[cn2 <= 1]) and M.worst_ratio(d2, ref2, cn2, A2) <= 1.0
    for z in (np.zeros(FULL[2:]), -np.zeros(FULL[2:], dtype=np.complex128)):
        d = ctx.tfm_model(s, s, z, R.FS, R.NT, t0=R.T0)
        parts = (d.real, d.imag) if np.iscomplexobj(d) else (d,)
        assert d.shape == (7, 7, R.NT) and all(not p.any() and not np.signbit(p).any() for p in parts)


def test_step_and_shape(ctx, envelope):
    T = R.fields(R.element_x(7))
    s = _put(ctx, T)
    x = M.noise_map(R.WINDOW_STEP3[2:], seed=22)
    d = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0, window=R.WINDOW_STEP3, step=3)
    ref, A, cn, _ = M.model_ref(T, T, x, R.NT, R.FS, R.T0, None, R.WINDOW_STEP3, 3)
    _check(envelope, "step3", d, ref, cn, A)
    f3 = R.full_window((R.NZ, R.NX), 3)
    x = M.noise_map(f3[2:], seed=23)
    d = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0, step=3)  # window None: the whole field at that step
    ref, A, cn, _ = M.model_ref(T, T, x, R.NT, R.FS, R.T0, None, None, 3)
    _check(envelope, "step3_full", d, ref, cn, A)
    small = (34, 66, 2, 3)
    x = M.noise_map(small[2:], seed=24, keep=1.0)
    d = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0, window=small)
    ref, A, cn, _ = M.model_ref(T, T, x, R.NT, R.FS, R.T0, None, small)
    _check(envelope, "window_2x3", d, ref, cn, A)
    # subgrid 3: fine shape 109 x 208
    assert ctx.field_shape(3) == (109, 208)
    T3 = R.fields(3 * R.element_x(7), nz=109, nx=208, dnx=R.DNX / 3)
    s3 = _put(ctx, T3, first=7, subgrid=3)
    x = M.noise_map((109, 208), seed=25)
    d = ctx.tfm_model(s3, s3, x, R.FS, R.NT, t0=R.T0, subgrid=3)
    ref, A, cn, _ = M.model_ref(T3, T3, x, R.NT, R.FS, R.T0)
    _check(envelope, "subgrid3", d, ref, cn, A)
    w3 = (5, 7, 33, 65)
    x = M.noise_map(w3[2:], seed=26)
    d = ctx.tfm_model(s3, s3, x, R.FS, R.NT, t0=R.T0, subgrid=3, window=w3, step=3)
    ref, A, cn, _ = M.model_ref(T3, T3, x, R.NT, R.FS, R.T0, None, w3, 3)
    _check(envelope, "subgrid3_step3", d, ref, cn, A)


def test_adjoint_identity(ctx, envelope):
    """<tfm(d), x> = <d, model(x)> with both sides run on the GPU: 65 x 65 pairs of noise data
    against the noise map, within tfm_model_ref.adjoint_bar."""
    T, x, _, _, _ = _case(65, 2)
    s = _put(ctx, T)
    d = R.data(65, 65)
    img = ctx.tfm(s, s, d, R.FS, t0=R.T0)
    m = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0)
    bar, N, S = M.adjoint_bar(T, T, d, x, R.FS, R.T0)
    lhs, rhs = M.inner(img, x), M.inner(d.astype(np.complex128), m)
    envelope["tfm_model/adjoint"] = abs(lhs - rhs) / bar
    print("tfm_model/adjoint: <tfm(d), x> = %.17g, <d, model(x)> = %.17g, difference %.3g, bar %.3g, N %d"
          % (lhs, rhs, abs(lhs - rhs), bar, N))
    assert N > 0 and abs(lhs - rhs) <= bar


def test_reproducibility(ctx, envelope):
    """Two calls agree within the bar (each is within it of the reference, and of each other);
    bit equality is not promised and not asserted."""
    T, x, ref, A, cn = _case(65, 2)
    s = _put(ctx, T)
    d1 = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0)
    d2 = ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0)
    _check(envelope, "repeat", d2, d1, cn, A)


def test_slots_untouched(ctx):
    T, x, _, _, _ = _case(7, 2)
    s = _put(ctx, T)
    before = [ctx.get_field(k, 1) for k in s]
    ctx.tfm_model(s, s, x, R.FS, R.NT, t0=R.T0)
    assert ctx.get_option("tfm_model_kernel_ms") > 0 and ctx.get_option("tfm_model_upload_ms") > 0
    for k in s:
        assert np.array_equal(ctx.get_field(k, 1), before[k]) and np.array_equal(before[k], T[k])


def _raw(ctx, subgrid, tx, rx, refl, ncomp, nt, t0, fs, w, win, step, out):
    """alifmm_tfm_model as declared, for the arguments the Python layer cannot express."""
    import _alifmm

    p = lambda a: None if a is None else a.ctypes.data
    rc = _alifmm.lib().alifmm_tfm_model(ctx._h, subgrid, len(tx) if tx is not None else 1, p(tx),
                                        len(rx) if rx is not None else 1, p(rx), p(refl), ncomp, nt, t0, fs, p(w), *win,
                                        step, p(out))
    ctx._chk(rc, "tfm_model")


def test_errors(ctx, envelope):
    """Every rejected input of test_gpu_tfm.py::test_errors in its modelling form, and NaN and inf
    in the map; nothing is written to the output, and a valid call passes afterwards."""
    import _alifmm

    E = _alifmm.AlifmmError
    T, x, ref, A, cn = _case(7, 2)
    s = _put(ctx, T)
    ctx.put_field(7, 3, np.zeros((109, 208)))
    kw = dict(t0=R.T0)
    z = lambda *shape: np.ones(shape, dtype=np.complex128)
    bare = _alifmm.Context(0)
    with pytest.raises(E, match="no model"):
        bare.tfm_model([0], [0], x, R.FS, R.NT, window=FULL)
    bare.close()
    xn, xi = x.copy(), x.copy()
    xn[36, 69] = complex(0.0, np.nan)
    xi[0, 0] = -np.inf
    bad = [
        lambda: ctx.tfm_model([0, 999], s, x, R.FS, R.NT, **kw),              # empty slot
        lambda: ctx.tfm_model(s, [-1] + s[1:], x, R.FS, R.NT, **kw),
        lambda: ctx.tfm_model(s, s[:6] + [7], x, R.FS, R.NT, **kw),           # mixed subgrids and shapes
        lambda: ctx.tfm_model(s, s, z(109, 208), R.FS, R.NT, subgrid=3, **kw),  # not the fields' subgrid
        lambda: ctx.tfm_model([], s, x, R.FS, R.NT, **kw),                    # ntx < 1
        lambda: ctx.tfm_model(s, [], x, R.FS, R.NT, **kw),                    # nrx < 1
        lambda: ctx.tfm_model(s, s, x, R.FS, 1, **kw),                        # nt < 2
        lambda: ctx.tfm_model(s, s, x, R.FS, 0, **kw),
        lambda: ctx.tfm_model(s, s, x, 0.0, R.NT, **kw),                      # fs
        lambda: ctx.tfm_model(s, s, x, -R.FS, R.NT, **kw),
        lambda: ctx.tfm_model(s, s, x, math.nan, R.NT, **kw),
        lambda: ctx.tfm_model(s, s, x, math.inf, R.NT, **kw),
        lambda: ctx.tfm_model(s, s, x, R.FS, R.NT, t0=math.nan),              # t0
        lambda: ctx.tfm_model(s, s, x, R.FS, R.NT, t0=-math.inf),
        lambda: ctx.tfm_model(s, s, x, R.FS, R.NT, step=0, **kw),             # step, niz, nix
        lambda: ctx.tfm_model(s, s, z(1, 1), R.FS, R.NT, step=0, window=(0, 0, 1, 1), **kw),
        lambda: ctx.tfm_model(s, s, z(0, 5), R.FS, R.NT, window=(0, 0, 0, 5), **kw),
        lambda: ctx.tfm_model(s, s, z(5, 0), R.FS, R.NT, window=(0, 0, 5, 0), **kw),
        lambda: ctx.tfm_model(s, s, z(R.NZ + 1, R.NX), R.FS, R.NT, window=(0, 0, R.NZ + 1, R.NX), **kw),  # outside
        lambda: ctx.tfm_model(s, s, z(R.NZ, R.NX + 1), R.FS, R.NT, window=(0, 0, R.NZ, R.NX + 1), **kw),
        lambda: ctx.tfm_model(s, s, z(5, 5), R.FS, R.NT, window=(-1, 0, 5, 5), **kw),
        lambda: ctx.tfm_model(s, s, z(5, 5), R.FS, R.NT, window=(0, -1, 5, 5), **kw),
        lambda: ctx.tfm_model(s, s, z(13, 23), R.FS, R.NT, window=(1, 2, 13, 23), step=3, **kw),
        lambda: ctx.tfm_model(s, s, z(2, 2), R.FS, R.NT, window=(5, 5, 2, 2), step=2 ** 30, **kw),
        lambda: ctx.tfm_model(s, s, xn, R.FS, R.NT, **kw),                    # a non-finite map value
        lambda: ctx.tfm_model(s, s, xi, R.FS, R.NT, **kw),
        lambda: ctx.tfm_model(s, s, np.where(x.real != 0, np.nan, 0.0), R.FS, R.NT, **kw),
    ]
    # the arguments only the C-ABI can express: ncomp, null pointers; the output stays as it was
    si = np.asarray(s, dtype=np.int32)
    xc = M.as_components(x)
    out = np.full((7, 7, R.NT, 2), 123.0)
    bad += [
        lambda: _raw(ctx, 1, si, si, xc, 3, R.NT, R.T0, R.FS, None, FULL, 1, out),
        lambda: _raw(ctx, 1, si, si, xc, 0, R.NT, R.T0, R.FS, None, FULL, 1, out),
        lambda: _raw(ctx, 1, None, si, xc, 2, R.NT, R.T0, R.FS, None, FULL, 1, out),
        lambda: _raw(ctx, 1, si, None, xc, 2, R.NT, R.T0, R.FS, None, FULL, 1, out),
        lambda: _raw(ctx, 1, si, si, None, 2, R.NT, R.T0, R.FS, None, FULL, 1, out),
        lambda: _raw(ctx, 1, si, si, xc, 2, R.NT, R.T0, R.FS, None, FULL, 1, None),
        lambda: _raw(ctx, 1, si, si, M.as_components(xn), 2, R.NT, R.T0, R.FS, None, FULL, 1, out),
        # a window whose extent passes 2^31 (validated in 64-bit, before the map is read)
        lambda: _raw(ctx, 1, si, si, xc, 2, R.NT, R.T0, R.FS, None, (5, 5, 2 ** 31 - 1, 2), 2 ** 31 - 1, out),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(E, match="rc=-2|tfm_model: step"):
            call()
            pytest.fail("rejected input %d was accepted" % k)
    assert (out == 123.0).all()
    # the Python layer's own checks
    with pytest.raises(ValueError):
        ctx.tfm_model(s, s, x[:5], R.FS, R.NT, **kw)
    with pytest.raises(ValueError):
        ctx.tfm_model(s, s, x, R.FS, R.NT, weights=np.ones((7, 6)), **kw)
    # the context is still usable: the valid call passes as in test_element_counts
    _raw(ctx, 1, si, si, xc, 2, R.NT, R.T0, R.FS, None, FULL, 1, out)
    _check(envelope, "after_errors_raw", out.view(np.complex128)[..., 0], ref, cn, A)
    _check(envelope, "after_errors", ctx.tfm_model(s, s, x, R.FS, R.NT, **kw), ref, cn, A)


def _pulse(fs, half=12):
    """Gaussian-windowed analytic wavelet at fs / 5, centred on sample `half`."""
    t = (np.arange(2 * half + 1) - half) / fs
    fc = fs / 5
    return np.exp(-2 * (fc * t) ** 2) * np.exp(2j * np.pi * fc * t), half


def test_end_to_end_through_the_dropin(envelope):
    """ALI_FMM.simulate_fmc on computed fields (the 61^2 Voronoi model of
    test_gpu_tfm.py::test_end_to_end_through_the_dropin): the data of one scatterer, before the
    pulse, are the reference's on update()'s fields; with a Gaussian-windowed pulse and imaged by
    ALI_FMM.tfm as complex64 they focus within one node of the scatterer.  The same round trip
    with the transmit path reflected off the last row."""
    import Anis_TTF_rays as A

    n, dnx, fs = 61, 1e-3, R.FS
    veln = W.voronoi_small(n, seed=7)
    velpn = np.zeros((n, n), dtype=np.int64)
    vm = np.ones((n, n))
    sd = W.stif_field(n, n)
    xs = np.arange(6, 56, 7)
    assert len(xs) == 8
    Mo = A.ALI_FMM(veln, velpn, vm, dnx * xs.astype(float), np.zeros(8), stif_den=sd, dnx=dnx)
    F = Mo.update(veln, velpn, vm, sd)
    q = (40, 23)
    x = np.zeros((n, n))
    x[q] = 1.0
    pulse, half = _pulse(fs)
    nt = math.ceil(2 * F.max() * fs) + 2 + len(pulse)
    d0 = Mo.simulate_fmc(x, fs, nt)
    ref, Am, cn, cnt = M.model_ref(F, F, x, nt, fs)
    assert cnt["inside"] == 64 and d0.dtype == np.float64
    _check(envelope, "dropin", d0, ref, cn, Am)
    d = Mo.simulate_fmc(x, fs, nt, pulse=pulse)
    assert d.shape == (8, 8, nt) and d.dtype == np.complex128
    conv = np.stack([[np.convolve(d0[a, b], pulse)[:nt] for b in range(8)] for a in range(8)])
    assert np.abs(d - conv).max() <= 1e-12 * np.abs(conv).max()
    img = Mo.tfm(d.astype(np.complex64), fs, t0=-half / fs)  # the pulse's centre delays the data by `half` samples
    a = np.abs(img)
    peak = np.unravel_index(a.argmax(), a.shape)
    print("peak %.1f at %s" % (a[peak], peak))
    assert abs(peak[0] - q[0]) <= 1 and abs(peak[1] - q[1]) <= 1 and a[peak] >= 0.5 * 64
    # element subsets and a complex map
    tx = [0, 2, 4, 6]
    xc = x * (0.5 - 2j)
    sub = Mo.simulate_fmc(xc, fs, nt, tx=tx)
    rsub, asub, csub, _ = M.model_ref(F[tx], F, xc, nt, fs)
    _check(envelope, "dropin_tx_subset", sub, rsub, csub, asub)
    with pytest.raises(IndexError, match="simulate_fmc"):
        Mo.simulate_fmc(x, fs, nt, tx=[8])
    with pytest.raises(ValueError, match="simulate_fmc"):
        Mo.simulate_fmc(x, fs, nt, tx_path="skip")
    # half-skip: transmit legs reflected off the last row
    wall = np.full(n, n - 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    q2 = (30, 35)
    x = np.zeros((n, n))
    x[q2] = 1.0
    probe = Mo.simulate_fmc(x, fs, 2, tx_path="skip", reflector=wall)  # computes the fields; the slots name them
    c, slots = Mo._ctx(0), Mo.skip_slots
    Tt = np.stack([c.get_field(slots["skip"][i], 1) for i in range(8)])
    Tr = np.stack([c.get_field(slots["direct"][i], 1) for i in range(8)])
    assert probe.shape == (8, 8, 2) and np.isfinite(Tt).all()
    nt = math.ceil((Tt.max() + Tr.max()) * fs) + 2 + len(pulse)
    d0 = Mo.simulate_fmc(x, fs, nt, tx_path="skip", reflector=wall)
    ref, Am, cn, cnt = M.model_ref(Tt, Tr, x, nt, fs)
    assert cnt["inside"] == 64
    _check(envelope, "dropin_half_skip", d0, ref, cn, Am)
    d = Mo.simulate_fmc(x, fs, nt, tx_path="skip", reflector=wall, pulse=pulse)
    img = Mo.tfm(d.astype(np.complex64), fs, t0=-half / fs, tx_path="skip", reflector=wall)
    a = np.abs(img)
    peak = np.unravel_index(a.argmax(), a.shape)
    print("half-skip peak %.1f at %s" % (a[peak], peak))
    assert abs(peak[0] - q2[0]) <= 1 and abs(peak[1] - q2[1]) <= 1
