"""One context through regrowth, release and re-creation of its device buffers (csrc/context.h
DevBuf): the TFM family, the resident operator and its solve run at 7 elements, at 65 (every
buffer regrows), at 7 again, once more after release_fields and put_field, and on a fresh context
after the first was destroyed.  The per-family tests reach these transitions only by accident of
their parameter order.

A 33 x 33 isotropic model at 5000 m/s, elements on row 0, straight-ray fields (tfm_ref.fields);
fs = 5 MHz and t0 = 0 put the delays of the 8 x 8 window inside nt = 48 and those of the 16 x 16
window inside nt = 96.  The rays of the operator join every element to every element's mirror on
the last row.

What the four runs at 7 elements must share.  The products whose sums have a fixed order agree bit
for bit: tfm, tfm(precision="f64"), tfm_coh (image, factor, sums), the operator's apply both ways
and its solve.  tfm_model and tfm_lsq add with atomics, so they agree within the bars of
test_gpu_tfm_model.py::test_reproducibility (tfm_model_ref.worst_ratio <= 1 against the first run,
with the restatement's counts and magnitudes) and of test_gpu_tfm_lsq.py::test_reproducibility
(tfm_lsq_ref.deviation <= 8 e_ref, e_ref being the converged restatement's deviation from numpy's
lstsq on the same problem, iterations equal here because max_iter stops both)."""
from types import SimpleNamespace

import numpy as np
import pytest

import sens_ref as SR
import tfm_lsq_ref as L
import tfm_model_ref as M
import tfm_ref as R
import workloads as W

pytestmark = pytest.mark.gpu

N = 33
FS, T0 = 5e6, 0.0
SMALL = (7, 48, (6, 12, 8, 8))
LARGE = (65, 96, (5, 9, 16, 16))


def _context():
    import _alifmm

    c = _alifmm.Context(0)
    c.set_model(np.zeros((N, N)), np.ones((N, N), dtype=np.int64), np.full((N, N), R.SPEED), None, W.default_table(),
                W.default_table(), R.DNX)
    return c


_cases = {}


def _case(shape):
    """Inputs of every call at (elements, nt, window); computed once, never modified."""
    if shape not in _cases:
        n, nt, win = shape
        xs = R.element_x(n, 1, N - 2)
        rng = np.random.default_rng(n)
        segs = [SimpleNamespace(x1=xa + 0.25, y1=0.5, x2=xb - 0.25, y2=N - 1.5) for xa in xs for xb in xs]
        ray_len, xy = SR.segments_request(segs)
        c = dict(T=R.fields(xs, N, N), d32=R.data(n, n, nt), d64=L.noise64(n, n, nt), x=M.noise_map(win[2:]),
                 ray_len=ray_len, xy=xy, xin=rng.standard_normal(N * N), yin=rng.standard_normal(len(segs)),
                 rhs=1e-6 * rng.standard_normal(len(segs)))
        for a in c.values():
            a.setflags(write=False)
        _cases[shape] = c
    return _cases[shape]


def _run(ctx, shape):
    """Every call of the sequence at one shape, the fields put first; the results by name."""
    n, nt, win = shape
    c = _case(shape)
    s = list(range(n))
    for k in s:
        ctx.put_field(k, 1, c["T"][k])
    out = {"tfm": ctx.tfm(s, s, c["d32"], FS, t0=T0, window=win),
           "tfm_f64": ctx.tfm(s, s, c["d64"], FS, t0=T0, window=win, precision="f64")}
    out["coh_image"], out["coh_factor"], out["coh_sums"] = ctx.tfm_coh(s, s, c["d32"], FS, t0=T0, window=win, sums=True)
    out["model"] = ctx.tfm_model(s, s, c["x"], FS, nt, t0=T0, window=win)
    out["lsq"], info = ctx.tfm_lsq(s, s, c["d64"], FS, t0=T0, window=win, damp=_damp(shape), max_iter=2, tol=0.0)
    assert info["iterations"] == 2 and info["reason"] == "max_iter"
    entries, _ = ctx.sens_op_build(c["ray_len"], c["xy"], subgrid=1, quantity=1)
    assert entries > 0 and ctx.get_option("sens_op_entries") == entries
    out["apply"] = ctx.sens_op_apply(c["xin"])
    out["apply_t"] = ctx.sens_op_apply(c["yin"], transpose=True)
    out["solve"], sinfo = ctx.sens_op_solve(c["rhs"], damp=1e-7, max_iter=2, tol=0.0)
    assert sinfo["iterations"] == 2 and sinfo["entries"] == entries
    for name, v in out.items():
        assert np.isfinite(v).all() and v.any(), name
    return out


_dense = {}


def _lsq_problem():
    """The dense operator of the small case, its damping (tfm_lsq_ref.DAMP sigma_max, as the solve
    cases of tfm_lsq_ref) and e_ref of the converged restatement."""
    if not _dense:
        n, nt, win = SMALL
        c = _case(SMALL)
        A = L.dense_A(c["T"], c["T"], nt, FS, T0, None, win, 1)
        D = L.difference(*win[2:])
        damp = L.DAMP * float(np.linalg.svd(A, compute_uv=False)[0])
        rhs = L.columns(c["d64"])
        x, info, _ = L.cgls(A, D, rhs, damp, 0.0, 1000, 1e-10)
        assert info["reason"] == "tol"
        _dense.update(damp=damp, e_ref=L.deviation(x, L.lstsq(A, D, rhs, damp, 0.0)))
    return _dense


def _damp(shape):
    return _lsq_problem()["damp"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_one_context_through_regrowth_release_and_recreation(envelope):
    n, nt, win = SMALL
    c = _case(SMALL)
    _, A, cn, cnt = M.model_ref(c["T"], c["T"], c["x"], nt, FS, T0, None, win)
    assert cnt["inside"] > 0
    e_ref = _lsq_problem()["e_ref"]
    ctx = _context()
    try:
        runs = {"first": _run(ctx, SMALL)}
        _run(ctx, LARGE)  # every buffer regrows
        runs["after_regrowth"] = _run(ctx, SMALL)
        ctx.release_fields()
        runs["after_release"] = _run(ctx, SMALL)
    finally:
        ctx.close()
    ctx = _context()
    try:
        runs["fresh_context"] = _run(ctx, SMALL)
    finally:
        ctx.close()
    first = runs.pop("first")
    for name, r in runs.items():
        for key in ("tfm", "tfm_f64", "coh_image", "coh_factor", "coh_sums", "apply", "apply_t", "solve"):
            assert r[key].shape == first[key].shape and np.array_equal(_bits(r[key]), _bits(first[key])), (name, key)
        ratio = M.worst_ratio(r["model"], first["model"], cn, A)
        dev = L.deviation(L.columns(r["lsq"]), L.columns(first["lsq"]))
        envelope["ctx_reuse/" + name] = {"model_worst_ratio": ratio, "lsq_deviation": dev, "e_ref": e_ref}
        print("ctx_reuse/" + name, envelope["ctx_reuse/" + name])
        assert ratio <= 1.0, (name, ratio)
        assert not r["model"][cn == 0].real.any() and not r["model"][cn == 0].imag.any()
        assert dev <= 8 * e_ref, (name, dev, e_ref)
