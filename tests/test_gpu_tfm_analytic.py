"""GPU tests of the RF front end of the imaging family through the drop-in class: ALI_FMM.analytic_fmc
and the analytic / band keywords of tfm(), tfm_coherence(), lsq_image() and sparse_image()
(alifmm_trace_spectral before the imaging call).  The model, the elements and the scatterer are those
of tests/test_gpu_tfm.py's drop-in test; the filter's bits are the numpy restatement's
(tests/trace_fft_ref.py), so the images are compared by equality."""
import math

import numpy as np
import pytest

import test_gpu_tfm as G
import tfm_ref as R
import trace_fft_ref as F
import workloads as W

pytestmark = pytest.mark.gpu

Q = (40, 23)  # the scatterer's node


@pytest.fixture(scope="module")
def case():
    """(M, fields, fs, rf): the drop-in model with its copied-out fields and real float32 RF, a tone
    burst per pair at T_a(Q) + T_b(Q)."""
    import Anis_TTF_rays as A

    n, dnx, fs = 61, 1e-3, R.FS
    veln = W.voronoi_small(n, seed=7)
    velpn = np.zeros((n, n), dtype=np.int64)
    vm = np.ones((n, n))
    sd = W.stif_field(n, n)
    xs = np.arange(6, 56, 7)
    M = A.ALI_FMM(veln, velpn, vm, dnx * xs.astype(float), np.zeros(8), stif_den=sd, dnx=dnx)
    fld = M.update(veln, velpn, vm, sd)
    tq = fld[:, Q[0], Q[1]]
    nt = math.ceil(2 * fld.max() * fs) + 2
    rf = np.ascontiguousarray(R.scatterer_data(tq, tq, fs, nt).real)
    assert rf.dtype == np.float32 and rf.shape == (8, 8, nt) and nt <= F.FFT_MAX
    for a in (fld, rf):
        a.setflags(write=False)
    return M, fld, fs, rf


def test_analytic_tfm_is_tfm_of_the_restatement(case, envelope):
    M, fld, fs, rf = case
    want_data = F.restatement(rf, None, True)
    data = M.analytic_fmc(rf)
    assert data.dtype == np.complex64 and np.array_equal(data, want_data)
    img = M.tfm(rf, fs, analytic=True)
    assert img.dtype == np.complex128 and np.array_equal(img, M.tfm(want_data, fs))
    # the envelope image peaks at the scatterer
    a = np.abs(img)
    peak = np.unravel_index(a.argmax(), a.shape)
    print("peak %.1f at %s" % (a[peak], peak))
    assert abs(peak[0] - Q[0]) <= 1 and abs(peak[1] - Q[1]) <= 1 and a[peak] >= 0.7 * 64
    # and it is the reference's image of the analytic data, at the bar of the TFM tests
    ref, mag, _ = R.tfm_ref(fld, fld, want_data, fs)
    G._check(envelope, "analytic_dropin", img, ref, 64, mag)


def test_pcf_on_rf(case):
    M, fld, fs, rf = case
    want_data = F.restatement(rf, None, True)
    img, fac = M.tfm_coherence(rf, fs, kind="pcf", analytic=True)
    img2, fac2 = M.tfm_coherence(want_data, fs, kind="pcf")
    assert np.array_equal(img, img2) and np.array_equal(fac, fac2)
    assert 0.0 <= fac.min() and fac.max() <= 1.0 and fac[Q] > 0.5
    import _alifmm

    with pytest.raises(_alifmm.AlifmmError):  # without the front end PCF still refuses real data
        M.tfm_coherence(rf, fs, kind="pcf")


def test_band_passes_through_the_response(case):
    """band= builds bandpass_response at the automatic length; the burst sits at fs / 5, inside."""
    import _alifmm

    M, fld, fs, rf = case
    nfft = 1 << (rf.shape[-1] - 1).bit_length()
    for band in ((0.1 * fs, 0.3 * fs), (0.1 * fs, 0.3 * fs, 0.02 * fs)):
        h = _alifmm.bandpass_response(nfft, fs, *band)
        want_data = F.restatement(rf, h, True)
        assert np.array_equal(M.analytic_fmc(rf, fs, band), want_data)
        img = M.tfm(rf, fs, analytic=True, band=band)
        assert np.array_equal(img, M.tfm(want_data, fs))
        a = np.abs(img)
        peak = np.unravel_index(a.argmax(), a.shape)
        assert abs(peak[0] - Q[0]) <= 1 and abs(peak[1] - Q[1]) <= 1


def test_defaults_change_nothing(case, envelope):
    """Without the keywords the real image is what it was: two calls agree to the bit and with the
    numpy reference at its existing bar."""
    M, fld, fs, rf = case
    img = M.tfm(rf, fs)
    assert img.dtype == np.float64 and np.array_equal(img, M.tfm(rf, fs))
    assert np.array_equal(img, M.tfm(rf, fs, analytic=False, band=None))
    ref, mag, _ = R.tfm_ref(fld, fld, rf, fs)
    G._check(envelope, "analytic_defaults", img, ref, 64, mag)


def test_solvers_take_the_keywords(case):
    """lsq_image and sparse_image run the same front end: their first gradient is that of the
    analytic data (the solves' sums have no fixed order, so this compares to rounding)."""
    M, fld, fs, rf = case
    want_data = F.restatement(rf, None, True)
    win = (Q[0] - 4, Q[1] - 4, 9, 9)
    for solve in (M.lsq_image, M.sparse_image):
        x1, i1 = solve(rf, fs, window=win, analytic=True, max_iter=2)
        x2, i2 = solve(want_data, fs, window=win, max_iter=2)
        assert x1.dtype == np.complex128 and x1.shape == (9, 9)
        for key in ("rhs_norm", "grad0"):
            assert i2[key] > 0 and abs(i1[key] - i2[key]) <= 1e-9 * i2[key], (solve.__name__, key)


def test_value_errors(case):
    M, fld, fs, rf = case
    cplx = F.restatement(rf, None, True)
    for call in (M.tfm, M.tfm_coherence, M.lsq_image, M.sparse_image):
        with pytest.raises(ValueError, match="complex"):
            call(cplx, fs, analytic=True)
        with pytest.raises(ValueError, match="band needs analytic"):
            call(rf, fs, band=(0.1 * fs, 0.3 * fs))
    with pytest.raises(ValueError, match="complex"):
        M.analytic_fmc(cplx)
    for band in ((-1.0, 0.3 * fs), (0.3 * fs, 0.1 * fs), (0.1 * fs, 0.6 * fs), (0.2 * fs, 0.2 * fs)):
        with pytest.raises(ValueError, match="band edges"):
            M.tfm(rf, fs, analytic=True, band=band)
    with pytest.raises(ValueError, match="band"):
        M.analytic_fmc(rf, fs, (0.1 * fs,))
    with pytest.raises(ValueError, match="fs"):
        M.analytic_fmc(rf, None, (0.1 * fs, 0.3 * fs))
