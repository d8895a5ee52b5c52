"""Pin the CPU oracle (oracle/alifmm_oracle.c) against vectors produced by the reference itself
(tests/golden/*.npz from oracle/gen_golden.py: numba 0.54, padded stage-1 semantics) and against the
published notebook outputs.  Bit-exact unless stated."""
import numpy as np
import pytest

import oracle as O
import workloads as W


def test_local_update_bitexact(golden):
    g = golden("local_ops")
    n = g["u_ttn"].shape[1]
    bad = 0
    for k in range(len(g["u_out"])):
        veln, velpn, vm = g["u_mat"][k]
        iz, ix, dnx, nnz_arg, nnx_arg = g["u_args"][k]
        sd = np.empty((n, n, 5), dtype=np.int64); sd[:, :] = g["u_stif"][k]
        v = O.update(np.full((n, n), veln), np.full((n, n), int(velpn)), np.full((n, n), vm), g["u_nsts"][k],
                     g["u_ttn"][k], int(iz), int(ix), dnx, int(nnz_arg), int(nnx_arg), g["tab_p"], sd)
        bad += v != g["u_out"][k]
    assert bad == 0


def test_local_fouds18_bitexact(golden):
    g = golden("local_ops")
    n = g["f_ttn"].shape[1]
    bad = 0
    for k in range(len(g["f_out"])):
        veln, velpn, vm = g["f_mat"][k]
        iz, ix, dnx = g["f_args"][k]
        sd = np.empty((n, n, 5), dtype=np.int64); sd[:, :] = g["f_stif"][k]
        v = O.fouds18_A(int(iz), int(ix), g["f_nsts"][k], g["f_ttn"][k], dnx, dnx, n, n, np.full((n, n), veln),
                        np.full((n, n), int(velpn)), np.full((n, n), vm), g["tab_g"], sd)
        bad += v != g["f_out"][k]
    assert bad == 0


def test_group_vel_bitexact(golden):
    g = golden("group_vel")
    a = np.array([O.group_vel(x, 249000, 133000, 205000, 125000, 7850, 1.0) for x in g["angles"]])
    b = np.array([O.group_vel(x, 203600, 129800, 203600, 133500, 7874, 1.3) for x in g["angles"]])
    assert np.array_equal(a, g["set1"]) and np.array_equal(b, g["iron_scaled"])


def test_time_between_points_bitexact(golden):
    rows = golden("tbp_weld")["rows"]
    veln, velpn, vm, sd = W.weld_model()
    vt = W.default_table()
    got = np.array([O.time_between_points(r[0], r[1], r[2], r[3], 2e-4, int(r[4]), vt, veln, velpn, vm, sd)
                    for r in rows])
    assert np.array_equal(got, rows[:, 5])


def test_fmm_small_bitexact(golden):
    g = golden("fmm_small")
    for k in range(int(g["ncases"])):
        p = "c%d_" % k
        dnx, x, z, sg = g[p + "meta"]
        stif = g[p + "stif"] if (p + "stif") in g else None
        args = (dnx * x, dnx * z, g[p + "veln"], g[p + "velpn"], g[p + "vel_map"], stif)
        if int(sg) == 1:
            T = O.travel(*args, g[p + "av"], g[p + "ph"], dnx=dnx)
        else:
            T = O.travel_finer_grid(*args, int(sg), g[p + "av"], g[p + "ph"], dnx=dnx)
        assert np.array_equal(T, g[p + "out"]), "case %d (src %s, sg %d)" % (k, (x, z), sg)


def test_c1_fields_bitexact_and_analytic(golden):
    g = golden("c1_fields")
    veln, velpn, vm, _ = W.c1_model()
    vt = W.default_table()
    zz, xx = np.mgrid[0:201, 0:201]
    for k, (x, z) in enumerate(g["src"]):
        T = O.travel(1e-3 * x, 1e-3 * z, veln, velpn, vm, None, vt, vt)
        assert np.array_equal(T, g["out"][k])
        r = np.hypot(zz - z, xx - x)
        m = r > 20
        rel = np.abs(T[m] - 1e-3 * r[m] / 5790.0) / (1e-3 * r[m] / 5790.0)
        # the reference's own discretisation error on C1: max 1.9e-2, mean <= 8.5e-3
        assert rel.max() < 2.0e-2 and rel.mean() < 9e-3


def test_weld_sg1_field_and_rays(golden):
    g = golden("weld_sg1")
    veln, velpn, vm, sd = W.weld_model()
    vt = W.default_table()
    scx, scz = W.weld_transducers()
    T = O.travel(scx[46], scz[46], veln, velpn, vm, sd, vt, vt, dnx=2e-4)
    assert np.array_equal(T, g["field"])
    isx, isz = np.round(scx / 2e-4), np.round(scz / 2e-4)
    for i in (0, 15, 30):
        rx, ry, t = O.find_ray(2e-4, vt, [isx[i], isz[i]], [isx[46], isz[46]], g["field"], veln, velpn, vm, sd, 1)
        assert np.array_equal(rx, g["ray_x_%d" % i]) and np.array_equal(ry, g["ray_y_%d" % i])
        assert t == float(g["time_%d" % i])


def test_weld_sg9_field_and_rays(golden):
    g = golden("weld_sg9")
    veln, velpn, vm, sd = W.weld_model()
    vt = W.default_table()
    scx, scz = W.weld_transducers()
    T = O.travel_finer_grid(scx[46], scz[46], veln, velpn, vm, sd, 9, vt, vt, dnx=2e-4)
    assert T.shape == tuple(g["fine_shape"])
    assert np.array_equal(T[::9, ::9], g["field_dec"])
    assert np.array_equal(T[T.shape[0] // 2], g["row_mid"]) and np.array_equal(T[:, T.shape[1] // 2], g["col_mid"])
    isx, isz = np.round(scx / 2e-4), np.round(scz / 2e-4)
    for i in (0, 15, 30):
        rx, ry, t = O.find_ray(2e-4, vt, [9 * isx[i], 9 * isz[i]], [9 * isx[46], 9 * isz[46]], T, veln, velpn, vm,
                               sd, 9)
        assert np.array_equal(rx, g["ray_x_%d" % i]) and np.array_equal(ry, g["ray_y_%d" % i])
        assert t == float(g["time_%d" % i])


def test_c3_2048_bitexact(golden):
    g = golden("c3_2048")
    veln, velpn, vm, sd = W.c3_model()
    x, z = W.c3_source()
    T = O.travel(x, z, veln, velpn, vm, sd, W.default_table(), W.default_table())
    assert np.array_equal(T[::8, ::8], g["field_dec8"]) and np.array_equal(T[682], g["row_src"])


def test_c4_weldlike_fields_and_rays(golden):
    g = golden("c4_weldlike")
    veln, velpn, vm, sd = W.weldlike_model()
    vt = W.default_table()
    dnx = W.weldlike_dnx()
    scx, scz = W.c4_sources(128)
    k = int(g["src_index"])
    T = O.travel(scx[k], scz[k], veln, velpn, vm, sd, vt, vt, dnx=dnx)
    assert np.array_equal(T[::8, ::8], g["field_dec8"]) and np.array_equal(T[0], g["row_top"])
    TR = O.travel(dnx * 2056, dnx * 4095, veln, velpn, vm, sd, vt, vt, dnx=dnx)
    assert np.array_equal(TR[::8, ::8], g["rec_field_dec8"])
    # the full-resolution windows around the source and the receiver (the GPU exact-prefix pin)
    w = golden("c4_window")
    for name, F in (("src", T), ("rec", TR)):
        z0, z1, x0, x1 = (int(v) for v in w[name + "_box"])
        assert np.array_equal(F[z0:z1, x0:x1], w[name + "_win"]), name
    for x in (8, 1032, 2056, 3080, 4088):
        rx, ry, t = O.find_ray(dnx, vt, [x, 0.0], [2056.0, 4095.0], TR, veln, velpn, vm, sd, 1)
        assert np.array_equal(rx, g["ray_x_%d" % x]) and np.array_equal(ry, g["ray_y_%d" % x])
        assert t == float(g["time_%d" % x])
    # the corridor fixture of the GPU ray pin (test_gpu_c5.py): the reference's own field values,
    # and the rays traced on the corridor alone are the reference's
    gc = golden("c4_ray_corridor")
    idx = gc["corridor_idx"]
    assert np.array_equal(TR.reshape(-1)[idx], gc["corridor_val"])
    TC = np.full(TR.size, np.nan)
    TC[idx] = gc["corridor_val"]
    TC = TC.reshape(TR.shape)
    for x in (8, 4088):
        rx, ry, t = O.find_ray(dnx, vt, [x, 0.0], [2056.0, 4095.0], TC, veln, velpn, vm, sd, 1)
        assert np.array_equal(rx, gc["ray_x_%d" % x]) and np.array_equal(ry, gc["ray_y_%d" % x])
        assert t == float(gc["time_%d" % x])


def _kat_rays(veln, velpn, vm, sd, vt, ph, scx, scz, pairs, sg, dnx=1e-3):
    isx, isz = np.round(scx / dnx), np.round(scz / dnx)
    out = {}
    for j in sorted(set(j for _, j in pairs)):
        T = O.travel_finer_grid(scx[j], scz[j], veln, velpn, vm, sd, sg, vt, ph, dnx=dnx)
        for (i, jj) in pairs:
            if jj == j:
                out[(i, j)] = O.find_ray(dnx, vt, [sg * isx[i], sg * isz[i]], [sg * isx[j], sg * isz[j]], T, veln,
                                         velpn, vm, sd, sg)
    return out


def test_notebook_kats(golden):
    """K1-K3: the notebook's published travel times (Ray tracing example.ipynb :305, :553-554, :733-734)."""
    g = golden("kat_notebook")
    dnx = 1e-3
    vt = W.default_table()
    # K1
    vm = np.zeros((201, 201)); vm[:, :] = 3000 + 21 * np.arange(201)[None, :]
    r = _kat_rays(np.zeros((201, 201)), np.ones((201, 201), dtype=np.int64), vm, np.zeros((201, 201, 5), np.int64),
                  vt, vt, dnx * np.array([1, 199]), dnx * np.array([30, 180]), [(0, 1)], 9)
    rx, ry, t = r[(0, 1)]
    assert t == g["k1_times"][0, 1]
    assert np.array_equal(rx / 9, g["k1_ray_x"]) and np.array_equal(ry / 9, g["k1_ray_y"])
    assert abs(t - 5.08845096e-05) / 5.08845096e-05 < 1e-8
    # K2 (first constant set; SURVEY B-D12)
    r = _kat_rays(np.zeros((201, 201)), np.ones((201, 201), dtype=np.int64), np.ones((201, 201)),
                  np.zeros((201, 201, 5), np.int64), g["k2_group"], g["k2_phase"], dnx * np.array([1, 199]),
                  dnx * np.array([100, 140]), [(0, 1), (1, 0)], 9)
    for (i, j) in [(0, 1), (1, 0)]:
        assert r[(i, j)][2] == g["k2_times"][i, j]
        assert np.array_equal(r[(i, j)][0] / 9, g["k2_ray_x_%d%d" % (i, j)])
    assert abs(r[(1, 0)][2] - 3.54107926e-05) / 3.54107926e-05 < 1e-8
    assert abs(r[(0, 1)][2] - 3.54124066e-05) / 3.54124066e-05 < 1e-4
    # K3
    sd = W.stif_field(201, 201)
    r = _kat_rays(20 * np.ones((201, 201)), np.zeros((201, 201), dtype=np.int64), np.ones((201, 201)), sd, vt, vt,
                  dnx * np.array([1, 199, 100]), dnx * np.array([100, 140, 1]), [(0, 1), (0, 2), (1, 2)], 9)
    pub = {(0, 1): 3.56081540e-05, (0, 2): 2.53646805e-05, (1, 2): 2.76255662e-05}
    for ij, tp in pub.items():
        assert r[ij][2] == g["k3_times"][ij]
        assert abs(r[ij][2] - tp) / tp < 5e-7


def test_band_case_matrix_preconditions():
    """What tests/test_gpu_band_small.py relies on, from the oracle alone (tests/band_cases.py): the
    CPU band model's field of every case and source of the matrix is finite and positive in every
    cell but the source (so the GPU test compares all cells, none masked); the models' material
    counts lie in the classes they are named for; the far-band case differs from the one-width
    field; a grid origin changes no bit; the dnz != dnx case runs."""
    import band_cases as BC

    for model in BC.MODELS:
        nz, nx = BC.MODEL_SHAPE[model]
        lo, hi = BC.MATERIAL_CLASS[model]
        assert lo <= BC.material_count(model, nz, nx) <= hi, model
    assert BC.material_count("many_mid", 61, 65) == 61 * 65 and BC.material_count("many_big", 97, 129) == 97 * 129
    # the band widths the library will pick: the default on one record and on grains, the narrow
    # one where the material changes from cell to cell
    assert BC.lib_options(BC.MODEL_CASES[0])["cdelta"] == 0.5 and BC.lib_options(BC.MODEL_CASES[1])["cdelta"] == 0.5
    for c in BC.MODEL_CASES[2:]:
        assert BC.lib_options(c)["cdelta"] == 0.2, c.name
    todo = BC.all_oracle_cases()
    assert len(set((c.name, s) for c, s in todo)) >= 300
    for c, s in todo:
        B = BC.model_field(c, s)
        assert B.shape == (c.nz, c.nx) and np.isfinite(B).all(), (c.name, s)
        assert B[s[1], s[0]] == 0.0 and (np.delete(B.ravel(), s[1] * c.nx + s[0]) > 0).all(), (c.name, s)
    far, one = BC.model_field(BC.FAR_CASE, BC.FAR_SOURCE), BC.model_field(BC.FAR_OFF_CASE, BC.FAR_SOURCE)
    assert int(np.sum(far != one)) > 10000  # the far band engages on most of the 129 x 129 grid
    for k in BC.PARAM_SOURCES:
        s = BC.sources(*BC.DEFAULT_SHAPE)[k]
        assert np.array_equal(BC.model_field(BC.ORIGIN_CASE, s), BC.model_field(BC.ORIGIN_ZERO, s)), s
    dz = [c for c in BC.PARAM_CASES if c.dnz != c.dnx]
    assert len(dz) == 1 and dz[0].dnz == 1.5e-3 and dz[0].dnx == 1e-3


def test_ray_case_matrix_preconditions():
    """What tests/test_gpu_rays_small.py relies on, from the oracle alone (tests/ray_cases.py).
    Every segment case is a 2-point ray on its pit field whose time is bit-equal to the same
    build's time_between_points; the piece and run classes are what the case names say and cover
    the ray kernel's edges (8 / 9 and 12 / 13 pieces, 4 / 5 runs, a run starting at piece 7, 8, 11,
    12 and 256, A B A, every record of the 256-record model); the models lie in the material
    classes they are named for; the walk cases have the lengths, flags and return codes their table
    states; and every case agrees between the glibc build and the correctly rounded one (lengths,
    flags and return codes equal, points within 1e-9, times within 1e-12), with no exception."""
    import ray_cases as RC

    builds = (O.LIB_GLIBC, O.LIB_CR)

    def agree(b):
        g, c = (RC.batch_reference(b, p) for p in builds)
        assert len(g) == len(c) == len(b.rays)
        for k, (a, d) in enumerate(zip(g, c)):
            assert (a.rc, a.early, a.walked) == (d.rc, d.early, d.walked), (b.name, k, a, d)
            assert len(a.x) == len(d.x) == a.walked and (a.rc < 0 or a.rc == a.walked), (b.name, k)
            assert np.max(np.abs(a.x - d.x)) <= 1e-9 and np.max(np.abs(a.y - d.y)) <= 1e-9, (b.name, k)
            assert abs(a.t - d.t) <= 1e-12 * abs(a.t), (b.name, k, a.t, d.t)
        return g

    # the models: record counts, and which of them the ray kernel keeps in LDS
    for name, (count, lds) in RC.SEG_MODELS.items():
        m = RC.model(name, *RC.SEG_H)
        n = RC.record_count(m)
        assert (100 < n <= 256) if count is None else n == count, (name, n)
        assert lds == (n <= 256 and RC.stiffness_rows(m) <= 64 and 361 * m.table.shape[1] <= 722), name
    assert sorted(set(RC.model("vt3", *RC.SEG_H).velpn.ravel())) == [0, 1, 2]
    assert RC.stiffness_rows(RC.model("stif65", *RC.SEG_H)) == 65
    assert np.array_equal(RC.model("stripes", *RC.SEG_V).ids, RC.model("stripes", *RC.SEG_H).ids.T)

    # the segments
    nseg = 0
    for mname, shape in RC.SEGMENT_RUNS:
        m = RC.model(mname, *shape)
        for sg in RC.SEG_SUBGRIDS:
            segs = RC.segments(shape, sg)
            keep, rsegs = RC.ray_segments(shape, sg)
            b = RC.segment_batch(mname, shape, sg)
            assert len(b.rays) == len(rsegs) and len(b.fields) <= 64
            agree(b)
            tg, tc = (RC.segment_times(mname, shape, sg, p) for p in builds)
            assert np.all(np.abs(tg - tc) <= 1e-12 * np.abs(tg)), (mname, shape, sg)
            for p, t in zip(builds, (tg, tc)):
                for k, s, r in zip(keep, rsegs, RC.batch_reference(b, p)):
                    assert r.rc == 2 and r.t == t[k], (mname, shape, sg, s.name, r.rc, r.t, t[k])
                    assert (r.x[0], r.y[0], r.x[1], r.y[1]) == (s.x1, s.y1, s.x2, s.y2), s.name
            for s in segs:
                assert abs(s.x1 - round(s.x1)) <= 0.4 and abs(s.y1 - round(s.y1)) <= 0.4, s.name  # off .5
                pieces, runs, starts, recs = RC.seg_classes(m, s, sg)
                if s.pieces is not None:
                    assert pieces == s.pieces, (mname, sg, s.name, pieces)
                if s.runs is not None and mname in ("stripes", "vt3"):
                    assert runs == s.runs, (mname, sg, s.name, runs)
                assert runs == 1 or mname != "iso"
            nseg += len(segs)
    assert nseg >= 4000  # 7 models x 2 subgrids x 272 segments on SEG_H, 2 x 2 x 95 on SEG_V
    for shape in (RC.SEG_H, RC.SEG_V):
        m = RC.model("stripes", *shape)
        for sg in RC.SEG_SUBGRIDS:
            segs = RC.segments(shape, sg)
            cl = [RC.seg_classes(m, s, sg) for s in segs if s.pieces is not None]
            assert {8, 9, 12, 13, 255, 256, 257} <= {c[0] for c in cl}
            assert {1, 2, 4, 5, 9, 10} <= {c[1] for c in cl}
            assert {7, 8, 11, 12, 256} <= {k for c in cl for k in c[2]}
            assert any(c[0] == 12 and c[2] == [11] for c in cl) and any(c[0] == 13 and c[2] == [12] for c in cl)
            assert any(c[3] == [1, 0, 1] for c in cl)  # A B A
            assert sum(s.pieces is None for s in segs) >= (200 if shape == RC.SEG_H else 24)
            assert sum(1 for s in segs if s.x1 == s.x2 and s.y1 == s.y2) >= 1
    m = RC.model("m256", *RC.SEG_H)
    seen = set()
    for s in RC.segments(RC.SEG_H, 1):
        seen.update(RC.seg_classes(m, s, 1)[3])
    assert len(seen) == 256  # whichever record the library numbers 255 lies on a tested segment

    # the walks: both builds agree; lengths from 2 points up; the thin grids' rays all complete
    for b in RC.WALK_BATCHES:
        g = agree(b)
        lens = [r.rc for r in g]
        assert min(lens) == 2 and max(lens) >= (25 if min(b.nz, b.nx) <= 3 else 55), (b.name, max(lens))
        assert b.sg > 3 or all(r.early == 0 for r in g) or min(b.nz, b.nx) <= 3, b.name
    assert all(max(r.rc for r in agree(b)) >= 70 for b in RC.DIST_BATCHES)
    g = agree(RC.DIAG_TIE_BATCH)
    assert all(r.rc >= 2 and r.early == 1 for r in g) and any(r.rc > 2 for r in g)
    # one case per exit of the walk (the table of the matrix)
    for b in RC.EXIT_BATCHES:
        g = dict(zip(RC.EXIT_NAMES, agree(b)))
        assert (g["early"].rc, g["early"].early) == (72, 1), b.name
        assert (g["leaves_grid"].rc, g["leaves_grid"].early) == (48, 0), b.name
        e = g["empty_plane"]
        assert (e.rc, e.early) == ((-4, 0) if b.sg >= 3 else (47, 0)) and e.walked >= 40, (b.name, e.rc, e.walked)
        for k in ("not_entered_same", "not_entered_1.5"):
            assert (g[k].rc, g[k].early) == (2, 0), (b.name, k)
        assert g["near_1.6"].rc == 2 and g["on_1.6"].rc == 2
    # the capacity ray and the list it is permuted in: lengths from 2 to the capacity
    g = agree(RC.MIX_BATCH)
    cap = g[RC.CAP_RAY]
    assert (cap.rc, cap.walked) == (-3, RC.CAP_POINTS - 1)
    # the orbit holds segments time_between_points() cannot walk (ray_cases.walk_cells): the reference
    # never times a ray cut short, and the device must not either
    endless = [k for k in range(cap.walked - 1)
               if RC.walk_cells(cap.x[k], cap.x[k + 1], cap.y[k], cap.y[k + 1], 1, limit=1000) is None]
    assert endless and all(cap.y[k] == cap.y[k + 1] and cap.y[k] % 2 == 1.5 for k in endless), endless[:5]
    assert min(r.walked for r in g) == 2 and sum(r.early for r in g) >= 1
    assert sum(1 for r in g if r.rc == 2) >= 2 and sum(1 for r in g if r.rc > 20) >= 8


def test_finer_case_matrix_preconditions(envelope):
    """What tests/test_gpu_finer_small.py relies on, from the correctly rounded build of the oracle
    alone (tests/finer_cases.py).  Every band-model field of the matrix is finite, zero at the
    source and positive elsewhere.  The model's exact region (T sg <= 0.999 tstop) equals the heap
    oracle bit for bit and holds at least 100 cells or the whole grid.  On the whole-field cases
    (2 x 2 .. 4 x 5, also at subgrid 11; 6 x 7 and 9 x 12 at subgrid 1) the model equals the heap
    oracle in every cell and hands no close node to the band.  The material classes are what the
    names say, many_* has a vel_map float32 does not hold, mixed at subgrid 3 gets a band width
    strictly inside (0.2, 0.5).  The far band changes more than a tenth of the cells at subgrid 3
    and none at subgrid 5 (far_sg 3).  Every case stays within the project's widest bar for the
    reformulation against the heap oracle (relative max 1e-2, mean 1e-3 beyond 5 sg fine nodes from
    the source; finer_cases.py names the two inputs replaced for it); no cell is masked out.  The
    deviation between the glibc and the correctly rounded build, and the peak heap entries per
    subgrid, are recorded (envelope "finer_cases/..."), not asserted.  One bounded search for a case
    whose heap passes the LDS walk's 4095 entries (the matrix's models at subgrid 9, exact_r 48)
    finds none: the largest peak is 1124, so exact_redo stays out of reach of this matrix."""
    import band_cases as BC
    import finer_cases as FC

    # material classes
    for c in FC.MODEL_CASES:
        lo, hi = BC.MATERIAL_CLASS[c.model]
        assert lo <= FC.material_count(c.model, c.nz, c.nx) <= hi, c.name
        vm = FC.model_arrays(c.model, c.nz, c.nx)[2]
        inexact = bool(np.any(vm.astype(np.float32).astype(np.float64) != vm))
        assert inexact == c.model.startswith("many_"), c.name
        veln = FC.model_arrays(c.model, c.nz, c.nx)[0]
        assert bool(np.any(veln != np.trunc(veln))) == (c.model != "iso"), c.name
    widths = {c.name: FC.lib_options(c)["cdelta"] for c in FC.MODEL_CASES}
    assert 0.2 < widths["mixed_sg3"] < 0.5 and widths["iso_sg3"] == 0.5 and widths["grain_sg9"] == 0.5
    assert all(FC.lib_options(c)["cdelta_far"] == 0.0 for c in FC.MODEL_CASES + [FC.FAR5_CASE])  # far_sg 1 / 3
    assert FC.lib_options(FC.FAR_CASE)["cdelta_far"] == 0.7 and FC.lib_options(FC.FAR_CASE)["r_far"] == 32
    assert [FC.fine_shape(c) for c in FC.MODEL_CASES[:3]] == [(70, 97), (116, 161), (208, 289)]
    assert len(FC.sources(*FC.DEFAULT_SHAPE)) == 9 and len(FC.sources(2, 2)) == 4

    todo = FC.all_model_cases()
    assert len(set((c.name, s) for c, s in todo)) >= 400
    peaks, dev = {}, {}
    for c, s in todo:
        B, info = FC.model_field(c, s)
        H = FC.heap_field(c, s)
        fz, fx = FC.fine_shape(c)
        isz, isx = s[1] * c.sg, s[0] * c.sg
        assert B.shape == H.shape == (fz, fx) and np.isfinite(B).all(), (c.name, s)
        assert B[isz, isx] == 0.0 and (np.delete(B.ravel(), isz * fx + isx) > 0).all(), (c.name, s)
        ex = FC.exact_region(c, s)
        assert np.array_equal(B[ex], H[ex]), (c.name, s)
        assert int(ex.sum()) >= min(100, B.size), (c.name, s, int(ex.sum()))
        zz, xx = np.mgrid[0:fz, 0:fx]
        far = np.hypot(zz - isz, xx - isx) > 5 * c.sg
        if far.any():
            rel = np.abs(B - H)[far] / H[far]
            assert rel.max() <= 1e-2 and rel.mean() <= 1e-3, (c.name, s, float(rel.max()), float(rel.mean()))
        peaks[c.sg] = max(peaks.get(c.sg, 0), info.peak1, info.peak2, info.peakp)
        assert info.pops >= 0 and info.close >= 0 and (info.pops > 0 or c.opts.get("exact_r") == 0), (c.name, s, info)
    for sg, p in peaks.items():
        envelope["finer_cases/heap_peak_sg%d" % sg] = p
    assert max(peaks.values()) <= 4000  # exact_redo is 0 on every case of the matrix

    # the whole field inside the prefix: the band starts from an empty close list
    for c in FC.WHOLE_CASES:
        for s in FC.case_sources(c):
            B, info = FC.model_field(c, s)
            assert np.array_equal(B, FC.heap_field(c, s)) and FC.exact_region(c, s).all(), (c.name, s)
            assert info.close == 0 and info.steps == 0, (c.name, s, info)
    L = O.open_lib(O.LIB_CR)
    for c in FC.SG1_CASES:
        o = BC.lib_options(BC.case(c.name, c.model, (c.nz, c.nx)))
        veln, velpn, vm, sd = FC.model_arrays(c.model, c.nz, c.nx)
        for s in FC.case_sources(c):
            x, z = FC.source_xy(c, s)
            B, steps = O.band_travel(x, z, veln, velpn, vm, sd, FC.TABLE, FC.TABLE, FC.model_vmax(c), cdelta=o["cdelta"],
                                     exact_init=True, r0=o["r0"], exact_r=o["exact_r"], cdelta_far=o["cdelta_far"],
                                     r_far=o["r_far"], lib=L)
            assert np.array_equal(B, FC.heap_field(c, s)) and steps[3] == 0, (c.name, s, steps)

    # the GPU test's bit-for-bit check of the exact region has teeth: a scaling by 1.0 / sg in place of
    # the division changes a share of the cells (by one ulp: invisible to both bars)
    for c in FC.MODEL_CASES[:3] + FC.HBM_CASES[:1]:
        s = FC.case_sources(c)[-1]
        t = FC.heap_field(c, s) * c.sg
        ex = FC.exact_region(c, s)
        assert int(np.sum((t * (1.0 / c.sg))[ex] != (t / c.sg)[ex])) >= 20, c.name

    # the far band: engaged at subgrid 3, off at subgrid 5
    for s in FC.case_sources(FC.FAR_CASE):
        a, b = FC.model_field(FC.FAR_CASE, s)[0], FC.model_field(FC.FAR_OFF_CASE, s)[0]
        assert int(np.sum(a != b)) > a.size // 10, (s, int(np.sum(a != b)))
        assert np.array_equal(FC.model_field(FC.FAR5_CASE, s)[0], FC.model_field(FC.FAR5_OFF_CASE, s)[0]), s
        assert np.array_equal(FC.model_field(FC.ORIGIN_CASE, s)[0], FC.model_field(FC.ORIGIN_ZERO, s)[0]), s

    # glibc against the correctly rounded build: recorded per case (one source each: the last)
    for c in FC.MODEL_CASES + FC.HBM_CASES + [FC.HBM13_CASE]:
        s = FC.case_sources(c)[-1]
        a, b = FC.model_field(c, s)[0], FC.model_field(c, s, build=O.LIB_GLIBC)[0]
        h, g = FC.heap_field(c, s), FC.heap_field(c, s, build=O.LIB_GLIBC)
        envelope["finer_cases/builds/" + c.name] = {
            "model_rel_max": float(np.max(np.abs(a - b) / np.maximum(a, 1e-300))),
            "heap_rel_max": float(np.max(np.abs(h - g) / np.maximum(h, 1e-300)))}

    # one bounded search for an exact_redo case: the matrix's models at subgrid 9 with exact_r 48
    best = 0
    for m in FC.MODELS:
        c = FC.case("redo_" + m, m, 9, FC.MODEL_SHAPE.get(m), opts={"exact_r": 48})
        for s in FC.sources(c.nz, c.nx)[-2:]:  # the near-edge and the interior node: the largest fronts
            info = FC.model_field(c, s)[1]
            best = max(best, info.peak1, info.peak2, info.peakp)
    envelope["finer_cases/redo_search_peak"] = best
    assert best <= FC.LDS_HEAP_ENTRIES  # none found: a case past it would join the matrix
