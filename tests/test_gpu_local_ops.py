"""Every device form of update() and fouds18_A() in csrc/local_ops.h against the correctly rounded
build of the oracle, bit for bit, on the designed case set of tests/local_ops_cases.py and on the
reference-made neighbourhoods of tests/golden/local_ops.npz.

  update():     op 0 (update_ref on the caller's patch), the register form (NbFieldT::load of the
                NaN-coded patch + update_nb: what fmm_seed, fmm_band_k and the walks' evaluation
                passes run) and the lane form (update_select_lanes over a wavefront, as fmm_init's
                relax role and fmm_exact_lds's relax_value run it)
  fouds18_A():  op 1 (all candidates on one lane), the four-lane form (fouds18_part 0..3, f18_min,
                fouds18_combine: fmm_band_k's fallback rounds), and both again with the material
                record and precomputed slownesses of a resident model (op 2, fouds18_part<true>)

Equality is the project's own claim (local_ops.h "any split gives the same bits",
"Bit-identical to update_ref"): no tolerance, no allowed share of exceptions.  The share of device
values that also equal the glibc build is recorded in the envelope, never asserted.
tests/test_local_ops_cases.py holds the preconditions (the set reaches the tie rule, the 1e6 limit,
every bounds combination, both exits of each operator)."""
import numpy as np
import pytest

import local_ops_cases as LC
import oracle as O
import workloads as W

pytestmark = pytest.mark.gpu

UPDATE_FORMS = (("op0", 0), ("register", 3), ("lane", 4))
FOUDS_FORMS = (("op1", 1), ("lanes4", 5))


@pytest.fixture(scope="module")
def ctx():
    import _alifmm

    c = _alifmm.Context(0)
    yield c
    c.close()


def _run(ctx, op, cs, mats, tab):
    """One form on every case of a set: the cases with a stiffness row and those without (None) go
    in separate calls, as the C ABI takes cell_stif for a whole batch."""
    veln, velpn, vm, stif_on, stif = mats
    out = np.full(len(cs.ttn), np.nan)
    for on in (True, False):
        k = np.flatnonzero(stif_on == on)
        if len(k):
            out[k] = ctx.local_ops(op, cs.ttn[k], cs.nsts[k], cs.iz[k], cs.ix[k], cs.dnx[k], cs.dnx[k], cs.nnz[k],
                                   cs.nnx[k], veln[k], velpn[k], vm[k], stif[k] if on else None, tab)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _compare(envelope, cs, forms, ref, glibc, describe):
    """forms: {name: values}.  Every form equals ref in every bit pattern; a mismatch names the form
    and prints its first 10 cases with every form's value."""
    bad = {}
    for name, v in forms.items():
        envelope["local_ops/%s/%s" % (cs.name, name)] = {
            "cases": len(v), "share_minus1": float(np.mean(v == -1.0)),
            "share_bit_equal_glibc": None if glibc is None else float(np.mean(_bits(v) == _bits(glibc)))}
        k = np.flatnonzero(_bits(v) != _bits(ref))
        if len(k):
            bad[name] = k
    for name, k in bad.items():
        print("%s: form %s differs from the oracle in %d of %d cases" % (cs.name, name, len(k), len(ref)))
        for c in k[:10]:
            print("  " + describe(c))
            print("    oracle %r  " % float(ref[c]) + "  ".join("%s %r" % (f, float(v[c])) for f, v in forms.items()))
    assert not bad, (cs.name, {name: len(k) for name, k in bad.items()})


@pytest.mark.parametrize("which", range(4))
def test_update_forms(ctx, envelope, which):
    cs = LC.update_sets()[which]
    forms = {name: _run(ctx, op, cs, LC.case_mats(cs), LC.TAB_P) for name, op in UPDATE_FORMS}
    _compare(envelope, cs, forms, LC.reference(cs), LC.reference(cs, O.LIB_GLIBC), lambda k: LC.describe(cs, k))


@pytest.mark.parametrize("which", range(2))
def test_fouds18_forms(ctx, envelope, which):
    cs = LC.fouds_sets()[which]
    forms = {name: _run(ctx, op, cs, LC.case_mats(cs), LC.TAB_G) for name, op in FOUDS_FORMS}
    _compare(envelope, cs, forms, LC.reference(cs), LC.reference(cs, O.LIB_GLIBC), lambda k: LC.describe(cs, k))


def test_golden_neighbourhoods(golden, ctx, envelope):
    g = golden("local_ops")
    u, f = LC.golden_sets(g)
    for cs, table, todo in ((u, g["tab_p"], UPDATE_FORMS), (f, g["tab_g"], FOUDS_FORMS)):
        mats = LC.golden_mats(g, cs)
        forms = {name: _run(ctx, op, cs, mats, table) for name, op in todo}
        _compare(envelope, cs, forms, LC.golden_reference(g, cs), LC.golden_reference(g, cs, O.LIB_GLIBC),
                 lambda k: "%s[%d] cell (%d, %d) nnz %d nnx %d material %r" % (cs.name, k, cs.iz[k], cs.ix[k], cs.nnz[k],
                                                                              cs.nnx[k], [a[k] for a in mats[:3]]))


def _resident(ctx, envelope, cs, tag):
    """Op 2 and its four-lane form on the two resident models, both material views."""
    vt = W.default_table()
    n = len(cs.ttn)
    for name, model, dx in LC.resident_models():
        veln, velpn, vm, sd = model
        ctx.set_model(veln, velpn, vm, sd, vt, vt, dx)
        mz, mx = LC.resident_cells(name, veln.shape, n)
        for quant in (0, 1):
            forms = {form: ctx.fouds18_band(cs.ttn, cs.nsts, cs.iz, cs.ix, cs.dnx, cs.dnx, cs.nnz, cs.nnx, mz, mx, quant,
                                            lanes=lanes) for form, lanes in (("op2", False), ("lanes4_pre", True))}
            ref = LC.resident_reference(name, model, quant, cs, mz, mx, vt)
            glibc = LC.resident_reference(name, model, quant, cs, mz, mx, vt, O.LIB_GLIBC)
            named = cs._replace(name="%s/%s_q%d" % (tag, name, quant))
            _compare(envelope, named, forms, ref, glibc,
                     lambda k: "%s[%d] cell (%d, %d) mask 0x%02x pattern %s field %d dnx %.17g model cell (%d, %d): veln "
                               "%.17g velpn %d vm %.17g" % (cs.name, k, cs.iz[k], cs.ix[k], cs.mask[k],
                                                            LC.PATTERNS[cs.pattern[k]], cs.field[k], cs.dnx[k], mz[k],
                                                            mx[k], veln[mz[k], mx[k]], velpn[mz[k], mx[k]],
                                                            vm[mz[k], mx[k]]))


def test_fouds18_resident_forms(ctx, envelope):
    _resident(ctx, envelope, LC.all_fouds(), "fouds18_all")


def test_fouds18_resident_forms_golden(golden, ctx, envelope):
    _resident(ctx, envelope, LC.golden_sets(golden("local_ops"))[1], "golden_fouds18")


def test_errors_leave_the_context_usable():
    """An unknown op, a NaN at a valid node and the resident-model forms without a model return
    ALIFMM_E_ARG (-2); one good call follows each."""
    import _alifmm

    E = _alifmm.AlifmmError
    cs = LC.update_sets()[0]
    k = np.arange(4095, 4095 + 64)  # the last plane-front mask and the first 63 of the all-tie field
    mats = [a[k] for a in LC.case_mats(cs)]
    ref = LC.reference(cs)[k]
    c = _alifmm.Context(0)
    try:
        def call(op, ttn=None, stif=mats[4]):
            return c.local_ops(op, cs.ttn[k] if ttn is None else ttn, cs.nsts[k], cs.iz[k], cs.ix[k], cs.dnx[k],
                               cs.dnx[k], cs.nnz[k], cs.nnx[k], mats[0], mats[1], mats[2], stif, LC.TAB_P)

        def good():
            # (one call with every case's stiffness row: the records that go without one are not compared)
            on = mats[3]
            assert np.array_equal(_bits(call(3)[on]), _bits(ref[on]))

        for op in (2, 6, 7, -1, 64):
            with pytest.raises(E, match="rc=-2"):
                call(op)
            good()
        v = np.flatnonzero(cs.nsts[k[5]].ravel() >= 0)[0]
        for bad in (np.nan, np.inf):
            t = cs.ttn[k].copy()
            t[5].ravel()[v] = bad
            for op in (3, 4):
                with pytest.raises(E, match="rc=-2"):
                    call(op, ttn=t)
            good()
        # a NaN at an invalid node is no error: it is what the coding puts there
        t = cs.ttn[k].copy()
        inv = cs.nsts[k] < 0
        t[inv] = np.nan
        on = mats[3]
        assert np.array_equal(_bits(call(3, ttn=t)[on]), _bits(ref[on]))
        f = LC.fouds_sets()[1]
        j = np.arange(32)
        z = np.zeros(32, dtype=np.int32)
        for lanes in (False, True):
            with pytest.raises(E, match="rc=-2"):
                c.fouds18_band(f.ttn[j], f.nsts[j], f.iz[j], f.ix[j], f.dnx[j], f.dnx[j], f.nnz[j], f.nnx[j], z, z, 0,
                               lanes=lanes)
            good()
        t = f.ttn[j].copy()
        t[3].ravel()[np.flatnonzero(f.nsts[j[3]].ravel() >= 0)[0]] = np.nan
        fm = [a[j] for a in LC.case_mats(f)]
        with pytest.raises(E, match="rc=-2"):
            c.local_ops(5, t, f.nsts[j], f.iz[j], f.ix[j], f.dnx[j], f.dnx[j], f.nnz[j], f.nnx[j], fm[0], fm[1], fm[2],
                        fm[4], LC.TAB_G)
        good()
    finally:
        c.close()
