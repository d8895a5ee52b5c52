"""The small-shape case matrix of the subgrid > 1 travel path (travel_finer_grid: fmm_exact_lds.hip /
fmm_exact.hip, fmm_band_k.hip mode 1, scale_kernel) against the CPU band model of that path
(oracle/band_model.c oband_travel_finer through oracle.band_travel_finer) and the heap oracle, both
from the correctly rounded build (oracle/lib/liboracle_cr.so: the device follows its functions, and
the heap oracle itself moves by 3.8e-4 between the two builds on many_mid 12 x 9, subgrid 11,
source (4, 6)).  Shared by tests/test_oracle.py (the model's side) and
tests/test_gpu_finer_small.py (the device's side).

The structure is tests/band_cases.py's: named cases, seeded models (band_cases.model_arrays),
sources as coarse nodes (ix, iz), cached read-only reference fields.  The matrix is a set of axes
around one default (coarse 24 x 33: fine 70 x 97 at subgrid 3, 116 x 161 at 5, 208 x 289 at 9, the
last stripe one column wide at stripe_log 3), not their product.
"""
import collections

import numpy as np

import band_cases as BC
import oracle as O
import workloads as W

TABLE = BC.TABLE
DEFAULT_SHAPE = (24, 33)
MODELS = BC.MODELS
SUBGRIDS = (3, 5, 9)

# the library's defaults (context.h)
LIB_DEFAULTS = {"cdelta": 0.5, "r0": 40.0, "exact_r": 20, "cdelta_far": -1.0, "r_far": 768.0, "far_sg": 1}
# the LDS walk's heap (fmm_exact_lds.hip kHeap = 4096 slots, 1-based): more entries -> error 9 -> the HBM walk
LDS_HEAP_ENTRIES = 4095

Case = collections.namedtuple("Case", "name model nz nx sg opts dnx dnz gox goz")


def case(name, model, sg, shape=None, opts=None, dnx=1e-3, dnz=None, gox=0.0, goz=0.0):
    nz, nx = DEFAULT_SHAPE if shape is None else shape
    return Case(name, model, nz, nx, sg, dict(opts or {}), dnx, dnx if dnz is None else dnz, gox, goz)


def fine_shape(c):
    return (c.sg * (c.nz - 1) + 1, c.sg * (c.nx - 1) + 1)


def cr():
    """The correctly rounded build of the oracle and the band model: the reference of this matrix."""
    return O.open_lib(O.LIB_CR)


def sources(nz, nx):
    """The nine coarse source nodes (ix, iz) of a grid: the four corners, two edge midpoints, a node
    one coarse cell from the left edge, a node two cells from the bottom edge and four from the right
    one, the interior.  The stage windows are 2.4 and 5.4 coarse cells wide at any subgrid: the two
    near-edge nodes clip the x9 window on one side only, and the second clips the x3 window on a side
    on which the x9 window is whole.  On the small grids they are clipped to the grid and those that
    coincide are dropped."""
    cx, cz = nx - 1, nz - 1
    s = [(0, 0), (cx, 0), (0, cz), (cx, cz),
         (nx // 2, 0), (0, nz // 2),
         (1, nz // 2 + 1), (cx - 4, 2),
         (nx // 3 + 2, (2 * nz) // 3)]
    out = []
    for x, z in s:
        p = (max(0, min(x, cx)), max(0, min(z, cz)))
        if p not in out:
            out.append(p)
    return out


def source_xy(c, src):
    return c.gox + c.dnx * src[0], c.goz + c.dnz * src[1]


# Two models of band_cases are replaced on the default grid, because there the band reformulation
# itself (not the device) leaves the project's widest bar against the heap oracle (relative max 1e-2
# beyond 5 sg fine nodes from the source; test_finer_case_matrix_preconditions holds every case to
# it).  With band_cases' grain crop (voronoi seed 5) the front of a corner or bottom-edge source
# runs along the grid's first row through one grain, and at the width 0.5 the model is 2.5e-2
# (subgrid 3), 3.3e-2 (5) and 4.5e-2 (9) above the heap oracle at the far end of that row; at the
# width 0.2 it equals the heap oracle bit for bit.  band_cases' many_* arrays for 24 rows (seed 24)
# give 1.7e-2 for the corner source (0, 0) at subgrid 3 (width 0.467).  The replacements are the
# same generators with another seed: two grains (voronoi seed 2: <= 5.8e-3 over the nine sources
# and the three subgrids) and per-cell materials (seed 1: <= 6.2e-3).  No case is masked out.
_REPLACED = {("grain", 24, 33): 2, ("many_mid", 24, 33): 1}
_models = {}


def model_arrays(model, nz, nx):
    """band_cases.model_arrays, but for the two replaced models (above); cached, never modified."""
    k = (model, nz, nx)
    if k not in _REPLACED:
        return BC.model_arrays(model, nz, nx)
    if k not in _models:
        sd = W.stif_field(nz, nx)
        if model == "grain":
            veln = np.ascontiguousarray(W.voronoi_small(129, seed=_REPLACED[k])[:nz, :nx])
            m = (veln, np.zeros((nz, nx), dtype=np.int64), np.ones((nz, nx)), sd)
        else:
            rng = np.random.default_rng(_REPLACED[k])
            veln = rng.uniform(0.0, 180.0, (nz, nx))
            m = (veln, np.zeros((nz, nx), dtype=np.int64), 1.0 + 0.2 * rng.random((nz, nx)), sd)
        for a in m:
            a.setflags(write=False)
        _models[k] = m
    return _models[k]


def material_count(model, nz, nx):
    veln, velpn, vm, sd = model_arrays(model, nz, nx)
    cols = [veln.ravel(), velpn.ravel().astype(np.float64), vm.ravel()]
    if sd is not None:
        cols += [sd[..., k].ravel().astype(np.float64) for k in range(5)]
    return len(np.unique(np.stack(cols, -1), axis=0))


_vmax = {}


def model_vmax(c):
    k = (c.model, c.nz, c.nx)
    if k not in _vmax:
        _, velpn, vm, sd = model_arrays(*k)
        _vmax[k] = BC.vmax_of(velpn, vm, sd, TABLE)
    return _vmax[k]


def band_cdelta(c):
    """context.h band_cdelta(ctx, sg): the option if set; else from the model's jump density
    divided by sg (the fraction per pair of the fine grid).  get_option("cdelta") answers for
    subgrid 1 only, so this restatement is the only source of the width at subgrid > 1."""
    if "cdelta" in c.opts:
        return float(c.opts["cdelta"])
    j = BC.jump_density(*model_arrays(c.model, c.nz, c.nx)) / c.sg
    return 0.5 if j <= 0.3 else 0.2 if j >= 0.6 else 0.5 + (0.2 - 0.5) * (j - 0.3) / (0.6 - 0.3)


def lib_options(c):
    """The band options in force for a case at its subgrid (context.h band_cdelta / band_cdelta_far,
    host_travel.cpp travel_chunk: the far band only when sg <= far_sg): what oracle.band_travel_finer is given."""
    o = dict(LIB_DEFAULTS)
    o.update({k: v for k, v in c.opts.items() if k in o})
    cd = band_cdelta(c)
    o["cdelta"] = cd
    far = o["cdelta_far"]
    far = 0.0 if far == 0 else 1.4 * cd if far < 0 else max(far, cd)
    o["cdelta_far"] = far if c.sg <= o["far_sg"] else 0.0
    return o


_fields = {}
_heap = {}


def _mkey(c, src):
    return (c.model, c.nz, c.nx, c.sg, c.dnx, c.dnz, c.gox, c.goz, tuple(src))


def model_field(c, src, vmax=None, build=None):
    """(field, FinerInfo) of the CPU band model for one source of a case, with the options in force
    (lib_options) and `vmax` as read back from a context (default: vmax_of).  Cached; read-only."""
    o = lib_options(c)
    vmax = model_vmax(c) if vmax is None else vmax
    build = O.LIB_CR if build is None else build
    key = _mkey(c, src) + (vmax, build, tuple(float(o[k]) for k in ("cdelta", "cdelta_far", "r_far", "r0", "exact_r")))
    if key not in _fields:
        veln, velpn, vm, sd = model_arrays(c.model, c.nz, c.nx)
        x, z = source_xy(c, src)
        B, info = O.band_travel_finer(x, z, veln, velpn, vm, sd, c.sg, TABLE, TABLE, vmax, cdelta=o["cdelta"],
                                      r0=o["r0"], exact_r=o["exact_r"], cdelta_far=o["cdelta_far"], r_far=o["r_far"],
                                      gox=c.gox, goz=c.goz, dnx=c.dnx, dnz=c.dnz, lib=O.open_lib(build))
        B.setflags(write=False)
        _fields[key] = (B, info)
    return _fields[key]


def heap_field(c, src, build=None):
    """The heap oracle's field (travel_finer_grid; travel at subgrid 1) of one source.  Cached."""
    build = O.LIB_CR if build is None else build
    key = _mkey(c, src) + (build,)
    if key not in _heap:
        veln, velpn, vm, sd = model_arrays(c.model, c.nz, c.nx)
        x, z = source_xy(c, src)
        L = O.open_lib(build)
        if c.sg == 1:
            H = O.travel(x, z, veln, velpn, vm, sd, TABLE, TABLE, gox=c.gox, goz=c.goz, dnx=c.dnx, dnz=c.dnz, lib=L)
        else:
            H = O.travel_finer_grid(x, z, veln, velpn, vm, sd, c.sg, TABLE, TABLE, gox=c.gox, goz=c.goz, dnx=c.dnx,
                                    dnz=c.dnz, lib=L)
        H.setflags(write=False)
        _heap[key] = H
    return _heap[key]


def tstop(c, vmax=None):
    """host_travel.cpp travel_chunk (P.tstop): the prefix's stop time, in the units of the field before the division by sg."""
    size2 = 2 * c.sg + (c.sg - 1) // 2 + 3 * c.sg
    return (size2 + lib_options(c)["exact_r"]) * c.dnx / (model_vmax(c) if vmax is None else vmax)


def exact_region(c, src, vmax=None):
    """The cells the heap-ordered prefix made known in the model: T sg <= 0.999 tstop (the margin keeps
    off the cells whose product rounds across tstop)."""
    B, _ = model_field(c, src, vmax)
    return B * c.sg <= 0.999 * tstop(c, vmax)


# ---- the matrix ----
# models x subgrids at the default geometry, nine sources.  many_big is on 65 x 65: the class its
# name states (more than 4096 records: no material ids at all) needs more than 4096 coarse cells
MODEL_SHAPE = {"many_big": (65, 65)}
MODEL_CASES = [case("%s_sg%d" % (m, sg), m, sg, MODEL_SHAPE.get(m)) for m in MODELS for sg in SUBGRIDS]
# shapes on iso and mixed: 2 x 2 (fine (sg + 1)^2: every window clipped on four sides), thin both
# ways, 4 x 5 (the whole field inside the prefix), 12 x 9, and 3 x 65 at subgrid 3 (fine 7 x 193:
# three 64-column stripes and one column)
SHAPES = ((2, 2), (2, 9), (9, 2), (4, 5), (12, 9))
SHAPE_CASES = [case("%s_%dx%d_sg%d" % (m, nz, nx, sg), m, sg, (nz, nx)) for m in ("iso", "mixed")
               for nz, nx in SHAPES for sg in SUBGRIDS]
SHAPE_CASES += [case("%s_3x65_sg3" % m, m, 3, (3, 65)) for m in ("iso", "mixed")]
# the whole fine field inside the exact prefix (the device equals the heap oracle in every cell):
# the 4 x 5 shape cases, and 4 x 5 at subgrid 11 (the HBM walk)
WHOLE_HBM_CASES = [case("%s_4x5_sg11" % m, m, 11, (4, 5)) for m in ("iso", "mixed")]
WHOLE_CASES = [c for c in SHAPE_CASES if (c.nz, c.nx) == (4, 5)] + WHOLE_HBM_CASES
# the HBM walk (af_exact_lds_fits is 0 from subgrid 11: its stage-1 grid is 487^2)
HBM_SOURCES = ((0, 0), (4, 6), (8, 5))
HBM_CASES = [case("%s_12x9_sg11" % m, m, 11, (12, 9)) for m in ("grain", "many_mid")]
HBM13_CASE = case("grain_12x9_sg13", "grain", 13, (12, 9))
HBM13_SOURCES = ((4, 6),)
# every parameter alone, three sources each: a corner, the near-edge node, the interior
PARAM_SOURCES = (0, 7, 8)
PARAM_CASES = [case("exact_r%d_sg%d" % (r, sg), "mixed", sg, opts={"exact_r": r}) for sg in (3, 9) for r in (0, 4, 48)]
PARAM_CASES += [
    case("cdelta01", "grain", 3, opts={"cdelta": 0.1}),
    case("r0_0", "grain", 3, opts={"r0": 0}),
    case("r0_10", "mixed", 3, opts={"r0": 10}),
    case("dnx2e-4", "grain", 3, dnx=2e-4),
    case("dnz15e-4", "grain", 3, dnx=1e-3, dnz=1.5e-3),
]
FAR_OPTS = {"far_sg": 3, "cdelta_far": 0.7, "r_far": 32}
FAR_CASE = case("far_sg3", "grain", 3, opts=FAR_OPTS)
FAR_OFF_CASE = case("far_off_sg3", "grain", 3)
FAR5_CASE = case("far_sg5", "grain", 5, opts=FAR_OPTS)  # sg 5 > far_sg 3: the far band stays off
FAR5_OFF_CASE = case("far_off_sg5", "grain", 5)
ORIGIN_CASE = case("origin", "grain", 3, gox=0.0125, goz=-0.003)
ORIGIN_ZERO = case("origin_zero", "grain", 3)
# members: stripe_log 3, K = 1 .. 16
MEMBER_CASES = [case("%s_members_sg%d" % (m, sg), m, sg) for m in ("mixed", "many_mid") for sg in (3, 5)]
MEMBER_SOURCES = (0, 3, 5, 7, 8)
# subgrid 1 on grids the whole of which lies inside the exact prefix (exact_r 20 nodes)
SG1_CASES = [case("%s_%dx%d_sg1" % (m, nz, nx), m, 1, (nz, nx)) for m in ("iso", "mixed", "many_mid")
             for nz, nx in ((6, 7), (9, 12))]


def case_sources(c):
    if c in HBM_CASES:
        return list(HBM_SOURCES)
    if c is HBM13_CASE:
        return list(HBM13_SOURCES)
    s = sources(c.nz, c.nx)
    if c in PARAM_CASES or c in (FAR_CASE, FAR_OFF_CASE, FAR5_CASE, FAR5_OFF_CASE, ORIGIN_CASE, ORIGIN_ZERO):
        return [s[k] for k in PARAM_SOURCES]
    return s


def all_model_cases():
    """(case, source) of every band-model field the GPU test compares with (subgrid > 1)."""
    out = []
    for c in (MODEL_CASES + SHAPE_CASES + WHOLE_HBM_CASES + HBM_CASES + [HBM13_CASE] + PARAM_CASES +
              [FAR_CASE, FAR_OFF_CASE, FAR5_CASE, FAR5_OFF_CASE, ORIGIN_CASE, ORIGIN_ZERO]):
        out += [(c, s) for s in case_sources(c)]
    return out
