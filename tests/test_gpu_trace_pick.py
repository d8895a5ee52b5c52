"""GPU tests of the time-of-flight picker (include/alifmm.h alifmm_trace_pick; csrc/trace_pick.hip,
the rules of csrc/trace_pick_term.h) against the numpy restatement tests/trace_pick_ref.py.  The
contract fixes every operation and the picks are maxima of a total order, so the comparisons are
equalities of bits, NaN positions included."""
import numpy as np
import pytest

import trace_fft_ref as FFT
import trace_pick_ref as R

pytestmark = pytest.mark.gpu

NAMES = {0: "peak", 1: "onset"}


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)  # no model: the picker needs none
    yield c
    c.close()


# ---- 1. bit equality against the restatement ----

@pytest.mark.parametrize("cplx,f32", R.TYPES)
def test_bits_against_the_restatement(ctx, cplx, f32):
    """Traces of 1, 2, 65 and 300 samples with the designed gates (1, 63, 64, 65 and 129 samples,
    touching both ends, equal maxima in different lanes, a plateau, zeros, NaN and inf, no gate,
    a larger sample just outside, onsets at the gate's edge), 1, 3, 5 and 67 of them (fewer than a
    workgroup's four wavefronts, not a multiple of it, several workgroups), both modes, frac 0.5
    and 1, guard 0 and 7; and one whole-trace gate of 8192 samples."""
    for nt, _ in R.SHAPES:
        for ntrace in (1, 3, 5, 67):
            data, lo, hi = R.case_set(nt, ntrace, cplx, f32)
            for mode, frac in R.MODES:
                for guard in R.GUARDS:
                    got = ctx.trace_pick(data, lo, hi, mode=NAMES[mode], frac=frac, guard=guard)
                    ok, why = R.same_bits(got, R.pick(data, lo, hi, mode, frac, guard))
                    assert ok, (nt, ntrace, mode, frac, guard, why)
    data, lo, hi = R.whole_trace_case(cplx, f32)
    for mode, frac in R.MODES:
        got = ctx.trace_pick(data, lo, hi, mode=NAMES[mode], frac=frac, guard=7)
        ok, why = R.same_bits(got, R.pick(data, lo, hi, mode, frac, 7))
        assert ok, (mode, frac, why)
    assert ctx.get_option("trace_pick_kernel_ms") > 0 and ctx.get_option("trace_pick_upload_ms") > 0
    assert ctx.get_option("trace_pick_download_ms") > 0 and ctx.get_option("trace_pick_filter_ms") == 0


def test_more_traces_than_wavefronts(ctx):
    """More traces than the launch has wavefronts: every wavefront walks its share with the grid's stride."""
    ntrace = 4 * int(ctx.get_option("trace_pick_grid")) + 3
    data = FFT.noise((ntrace, 9), True, 21, f32=True)
    lo = (np.arange(ntrace) % 5).astype(np.int32)
    hi = (9 - np.arange(ntrace) % 3).astype(np.int32)
    ok, why = R.same_bits(ctx.trace_pick(data, lo, hi, guard=2), R.pick(data, lo, hi, 0, 0.5, 2))
    assert ok, why


# ---- 2. the resident filter: filter 1 is trace_spectral followed by filter 0 ----

@pytest.mark.parametrize("f32", (False, True))
def test_filtered_picks_are_picks_of_the_filtered(ctx, f32):
    for nt, nfft in ((300, None), (300, 1024), (1000, None), (1000, 2048)):
        n = nfft or 1 << (nt - 1).bit_length()
        x = FFT.noise((5, nt), False, 80 + nt, f32=f32)
        lo = np.array([0, 10, nt - 70, 33, 50], dtype=np.int32)
        hi = np.array([nt, 139, nt, 33, 114], dtype=np.int32)
        for response in (None, FFT.noise_response(n, 2), FFT.noise_response(n, 1)):
            y = ctx.trace_spectral(x, response=response, analytic=True, nfft=nfft)
            assert np.array_equal(y, FFT.restatement(x, response, True, nfft))
            for mode, frac in R.MODES:
                got = ctx.trace_pick(x, lo, hi, mode=NAMES[mode], frac=frac, guard=3, response=response, analytic=True,
                                     nfft=nfft)
                assert ctx.get_option("trace_pick_filter_ms") > 0
                ok, why = R.same_bits(got, ctx.trace_pick(y, lo, hi, mode=NAMES[mode], frac=frac, guard=3))
                assert ok, (nt, nfft, mode, why)
                ok, why = R.same_bits(got, R.pick(y, lo, hi, mode, frac, 3))
                assert ok, (nt, nfft, mode, why)
    # a response without the mask, on complex data
    xc = FFT.noise((3, 300), True, 90, f32=f32)
    h = FFT.noise_response(512, 2)
    got = ctx.trace_pick(xc, 5, 290, response=h)
    ok, why = R.same_bits(got, R.pick(FFT.restatement(xc, h, False), np.full(3, 5), np.full(3, 290)))
    assert ok, why


# ---- 3. trace independence, repeatability ----

def test_trace_independence(ctx):
    data, lo, hi = R.case_set(300, 67, True, False, seed=3)
    first = ctx.trace_pick(data, lo, hi, mode="onset", frac=0.3, guard=5)
    ok, why = R.same_bits(ctx.trace_pick(data, lo, hi, mode="onset", frac=0.3, guard=5), first)  # a second call's bits
    assert ok, why
    p = np.random.default_rng(4).permutation(67)
    ok, why = R.same_bits(ctx.trace_pick(data[p], lo[p], hi[p], mode="onset", frac=0.3, guard=5), [a[p] for a in first])
    assert ok, why
    for k in (0, 13, 66):  # a trace alone has the bits it has among the others
        ok, why = R.same_bits(ctx.trace_pick(data[k], lo[k], hi[k], mode="onset", frac=0.3, guard=5), [a[k] for a in first])
        assert ok, (k, why)
    # leading dimensions of any shape
    cube = data[:60].reshape(3, 4, 5, 300)
    got = ctx.trace_pick(cube, lo[:60].reshape(3, 4, 5), hi[:60].reshape(3, 4, 5), mode="onset", frac=0.3, guard=5)
    ok, why = R.same_bits(got, [a[:60].reshape(3, 4, 5) for a in first])
    assert ok, why


# ---- 4. errors ----

def _raw(ctx, ntrace, nt, ncomp, dtype, inp, filt, nfft, resp_comp, resp, analytic, lo, hi, mode, frac, guard, outs):
    """alifmm_trace_pick as declared, for the arguments the Python layer cannot express."""
    import _alifmm

    p = lambda a: None if a is None else a.ctypes.data
    rc = _alifmm.lib().alifmm_trace_pick(ctx._h, ntrace, nt, ncomp, dtype, p(inp), filt, nfft, resp_comp, p(resp), analytic,
                                         p(lo), p(hi), mode, frac, guard, *[p(o) for o in outs])
    ctx._chk(rc, "trace_pick")


def test_errors(ctx):
    """Every rejected input of the contract raises with rc=-2 and leaves the outputs as they were;
    valid calls pass afterwards, and trace_spectral's bits are those from before."""
    import _alifmm

    E = _alifmm.AlifmmError
    nt = 50
    x = FFT.noise((3, nt), False, 61)
    h1 = FFT.noise_response(64, 1)
    hnan = h1.copy()
    hnan[7] = np.nan
    before = ctx.trace_spectral(x, response=h1, analytic=True)
    lo, hi = np.array([0, 10, 20], dtype=np.int32), np.array([50, 40, 20], dtype=np.int32)
    neg, far = np.array([0, -1, 20], dtype=np.int32), np.array([50, 51, 20], dtype=np.int32)
    outs = [np.full(3, 123.0), np.full(3, 123.0), np.full(3, 123, dtype=np.int32), np.full(3, 123.0),
            np.full(3, 123, dtype=np.int32), np.full(3, 123, dtype=np.int32)]

    def call(ntrace=3, nt=nt, ncomp=1, dtype=0, inp=x, filt=0, nfft=0, resp_comp=0, resp=None, analytic=0, lo=lo, hi=hi,
             mode=0, frac=0.5, guard=0, outs=outs):
        _raw(ctx, ntrace, nt, ncomp, dtype, inp, filt, nfft, resp_comp, resp, analytic, lo, hi, mode, frac, guard, outs)

    bad = [dict(inp=None), dict(lo=None), dict(hi=None)]
    bad += [dict(outs=outs[:k] + [None] + outs[k + 1:]) for k in range(6)]                  # null pointers
    bad += [dict(ntrace=0), dict(ntrace=-1), dict(nt=0), dict(nt=-5), dict(ntrace=2 ** 62)]
    bad += [dict(ncomp=0), dict(ncomp=3), dict(dtype=-1), dict(dtype=2), dict(filt=-1), dict(filt=2), dict(mode=-1), dict(mode=2)]
    bad += [dict(mode=1, frac=0.0), dict(mode=1, frac=-0.5), dict(mode=1, frac=1.5), dict(mode=1, frac=np.nan), dict(guard=-1)]
    bad += [dict(lo=neg), dict(hi=far)]                                                       # a gate that leaves the trace
    bad += [dict(nfft=64), dict(resp_comp=1, resp=h1), dict(resp=h1), dict(analytic=1)]       # filter 0 takes no filter arguments
    # filter 1: alifmm_trace_spectral's refusals
    bad += [dict(filt=1, analytic=1, nfft=32), dict(filt=1, analytic=1, nfft=96), dict(filt=1, analytic=1, nfft=16384),
            dict(filt=1, analytic=2), dict(filt=1, analytic=-1), dict(filt=1, resp_comp=3, resp=h1, nfft=64),
            dict(filt=1, resp_comp=1, nfft=64), dict(filt=1, resp=h1, nfft=64), dict(filt=1, resp_comp=1, resp=hnan, nfft=64),
            dict(filt=1, analytic=1, ntrace=1, nt=8193, inp=np.zeros((1, 8193)), lo=lo[:1], hi=hi[:1])]
    for k, kw in enumerate(bad):
        with pytest.raises(E, match="rc=-2"):
            call(**kw)
            pytest.fail("rejected input %d %r was accepted" % (k, kw))
        assert all((o == 123).all() for o in outs), kw
    assert _alifmm.lib().alifmm_trace_pick(None, 3, nt, 1, 0, x.ctypes.data, 0, 0, 0, None, 0, lo.ctypes.data, hi.ctypes.data,
                                           0, 0.5, 0, *[o.ctypes.data for o in outs]) == -2
    assert all((o == 123).all() for o in outs)
    # the Python layer's own checks
    with pytest.raises(ValueError, match="shape"):
        ctx.trace_pick(np.float64(1.0), 0, 1)
    with pytest.raises(ValueError, match="mode"):
        ctx.trace_pick(x, lo, hi, mode="valley")
    with pytest.raises(ValueError, match="gates"):
        ctx.trace_pick(x, lo[:2], hi[:2])
    with pytest.raises(ValueError, match="response"):
        ctx.trace_pick(x, lo, hi, response=np.ones(32))
    with pytest.raises(ValueError, match="nfft"):
        ctx.trace_pick(x, lo, hi, nfft=64)
    with pytest.raises(E, match="rc=-2"):
        ctx.trace_pick(x, lo, hi, mode="onset", frac=2.0)
    # the context is still usable: the raw call, the method, and the filter's bits from before
    call()
    want = R.pick(x, lo, hi)
    ok, why = R.same_bits([outs[k] for k in range(6)], want)
    assert ok, why
    call(filt=1, nfft=64, resp_comp=1, resp=h1, analytic=1)
    ok, why = R.same_bits(outs, R.pick(before, lo, hi))
    assert ok, why
    assert np.array_equal(ctx.trace_spectral(x, response=h1, analytic=True), before)
    ok, why = R.same_bits(ctx.trace_pick(x, lo, hi), want)
    assert ok, why


# ---- 5. end to end: picked times into a tomography step ----

def test_end_to_end_pick_times():
    """A 41 x 41 model of two materials (3000 m/s over 4500 m/s), four elements on the top row facing
    four on the bottom row.  The times of the "true" model place one sampled Gaussian pulse (sigma 6
    samples, 0.1 cycles per sample) per pair; pick_times gated around the times of a start model
    whose vel_map is 2 % off returns the true times within 0.01 sample, the condition
    tests/test_trace_pick_ref.py checks for the rule on such pulses (plus the rounding of the
    conversions between seconds and samples, 1e-9 sample), NaN with flag 1 for the pairs not asked
    for, and picked - start feeds tomography_step."""
    import Anis_TTF_rays as A

    n, dnx, fs, nt = 41, 1e-3, 50e6, 1024
    veln = np.zeros((n, n))
    velpn = np.ones((n, n), dtype=int)
    vm = np.full((n, n), 3000.0)
    vm[n // 2:] = 4500.0
    scx = dnx * np.array([8.0, 16.0, 24.0, 32.0, 8.0, 16.0, 24.0, 32.0])
    scz = dnx * np.array([0.0, 0.0, 0.0, 0.0, 40.0, 40.0, 40.0, 40.0])
    pairs = np.zeros((8, 8))
    pairs[:4, 4:] = 1
    asked = pairs == 1

    def model(vel_map):
        M = A.ALI_FMM(veln, velpn, vel_map, scx, scz, dnx=dnx)
        return M, M.find_all_TTF_rays(veln, velpn, vel_map, subgrid_size=3, trans_pairs=pairs)

    _, true = model(vm)
    M, start = model(1.02 * vm)
    shift = np.abs(true - start)[asked].max()
    assert 2.0 / fs < shift < 0.4e-6  # the start model is off by several samples
    k = np.arange(nt)[None, None, :] - (true * fs)[:, :, None]
    rf = np.where(asked[:, :, None], np.exp(-0.5 * (k / 6.0) ** 2) * np.cos(2 * np.pi * 0.1 * k), 0.0)
    around = np.where(asked, start, np.nan)
    picked, info = M.pick_times(rf, fs, around=around, half_width=0.5e-6)
    err = np.abs(picked - true)[asked].max() * fs
    print("end to end: max |picked - true| = %.4g sample, shift %.3g samples" % (err, shift * fs))
    assert err <= 0.01 + 1e-9
    assert np.isnan(picked[~asked]).all() and (info["flags"][~asked] == 1).all() and (info["flags"][asked] == 0).all()
    assert (info["idx"][~asked] == -1).all() and np.isnan(info["ratio"][~asked]).all()
    assert (info["ratio"][asked] > 0.9).all() and (info["ratio"][asked] < 1).all()  # guard 0: the peak's neighbour
    assert (np.abs(info["pos"][asked] - (true * fs)[asked]) <= 0.01 + 1e-9).all()
    # float32 RF and a guard that skips the pulse: the same picks to the rule's accuracy, no runner-up of weight
    # (rounding the samples to float32 moves an amplitude by 6e-8 of the peak and the vertex by that over the
    # parabola's curvature, 1 / sigma^2 = 1 / 36 of the peak: 2e-6 sample, 1e-4 allowed; beyond 30 samples = 5 sigma
    # the envelope is below exp(-12.5) = 4e-6 of the peak)
    p32, i32 = M.pick_times(rf.astype(np.float32), fs, around=around, half_width=0.5e-6, guard=30)
    assert np.abs(p32 - true)[asked].max() * fs <= 0.01 + 1e-4 and (i32["ratio"][asked] < 1e-3).all()
    valid = [(int(i), int(j)) for i, j in zip(*np.nonzero(asked))]
    delta, sol = M.tomography_step(picked - start, param="vel_map", damp=1e-7, smooth=1e-7, pairs=valid)
    assert delta.shape == (n, n) and np.isfinite(delta).all() and delta.any() and sol["iterations"] >= 1
