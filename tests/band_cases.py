"""The small-shape case matrix of the band kernel (fmm_band_k.hip) against the CPU band model
(oracle/band_model.c through oracle.band_travel), shared by tests/test_oracle.py (the model's side:
every case is finite, the material classes are what their names say) and tests/test_gpu_band_small.py
(the device's side: every cell of every case within 1e-9 of the model).

Everything is deterministic: seeded generators, sources given as grid nodes.  A case is a model on
a grid, the library options set before set_model, the spacing and the origin; its sources are grid
nodes (ix, iz).  The matrix is a set of axes around one default (97 x 129, the library's own
options), not their product.
"""
import collections

import numpy as np

import oracle as O
import workloads as W

TABLE = W.default_table()

# nz x nx.  129 columns: the last stripe is one column wide at every stripe width; 127: it is one
# column short; 2 rows / 3 columns: the stencils hang over the grid on both sides
SHAPES = ((97, 129), (129, 97), (61, 65), (41, 127), (2, 65), (65, 3))
DEFAULT_SHAPE = (97, 129)
MODELS = ("iso", "grain", "mixed", "many_mid", "many_big")
MODEL_SHAPE = {"iso": DEFAULT_SHAPE, "grain": DEFAULT_SHAPE, "mixed": DEFAULT_SHAPE, "many_mid": (61, 65),
               "many_big": DEFAULT_SHAPE}
# distinct (veln, velpn, vm, stiffness) records: one; the LDS table with byte ids; ids and records
# in HBM; no ids at all (fmm_band_k.hip af_launch_band_k, band_common.h band_mat)
MATERIAL_CLASS = {"iso": (1, 1), "grain": (2, 256), "mixed": (101, 256), "many_mid": (257, 4096),
                  "many_big": (4097, 1 << 62)}

# the library's defaults (context.h) and its automatic band width (band_cdelta / band_cdelta_far)
LIB_DEFAULTS = {"cdelta": 0.5, "r0": 40.0, "exact_r": 20, "cdelta_far": -1.0, "r_far": 768.0}

Case = collections.namedtuple("Case", "name model nz nx opts dnx dnz gox goz")


def case(name, model, shape=None, opts=None, dnx=1e-3, dnz=None, gox=0.0, goz=0.0):
    nz, nx = MODEL_SHAPE[model] if shape is None else shape
    return Case(name, model, nz, nx, dict(opts or {}), dnx, dnx if dnz is None else dnz, gox, goz)


def vmax_of(velpn, vm, sd, vt):
    """host_model.cpp set_model's vmax: the fastest group velocity over the model."""
    ang = 0.05 * np.arange(3601)
    rows = {}
    v = 0.0
    for i in np.ndindex(velpn.shape):
        if velpn[i] != 0:
            v = max(v, vt[:181, velpn[i]].max() * vm[i])
        else:
            key = tuple(sd[i])
            if key not in rows:
                rows[key] = max(O.group_vel(a, *[float(k) for k in key]) for a in ang)
            v = max(v, rows[key] * vm[i])
    return v


def jump_density(veln, velpn, vm, sd):
    """Fraction of 4-neighbour pairs whose materials differ (host_model.cpp set_model's jump)."""
    key = [veln, vm, velpn.astype(np.float64)]
    if sd is not None:
        key += [sd[..., k].astype(np.float64) for k in range(5)]
    key = np.stack(key, -1)
    dh = np.any(key[:, 1:] != key[:, :-1], -1)
    dv = np.any(key[1:, :] != key[:-1, :], -1)
    return float((dh.sum() + dv.sum()) / (dh.size + dv.size))


_models = {}


def model_arrays(model, nz, nx):
    """(veln, velpn, vel_map, stif_den) of a named model on an nz x nx grid; cached, never modified."""
    k = (model, nz, nx)
    if k in _models:
        return _models[k]
    sd = W.stif_field(nz, nx)
    if model == "iso":
        m = (np.zeros((nz, nx)), np.ones((nz, nx), dtype=np.int64), np.full((nz, nx), 5790.0), None)
    elif model == "grain":
        veln = np.ascontiguousarray(W.voronoi_small(129, seed=5)[:nz, :nx])
        m = (veln, np.zeros((nz, nx), dtype=np.int64), np.ones((nz, nx)), sd)
    elif model == "mixed":
        rng = np.random.default_rng(3)
        veln = rng.integers(0, 100, (nz, nx)).astype(np.float64) * 1.7
        velpn = (rng.random((nz, nx)) < 0.3).astype(np.int64)
        m = (veln, velpn, np.where(velpn == 1, 5790.0, 1.0), sd)
    elif model in ("many_mid", "many_big"):
        rng = np.random.default_rng(nz)
        veln = rng.uniform(0.0, 180.0, (nz, nx))
        m = (veln, np.zeros((nz, nx), dtype=np.int64), 1.0 + 0.2 * rng.random((nz, nx)), sd)
    else:
        raise KeyError(model)
    for a in m:
        if a is not None:
            a.setflags(write=False)
    _models[k] = m
    return m


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
        _vmax[k] = vmax_of(velpn, vm, sd, TABLE)
    return _vmax[k]


def lib_options(c):
    """The band options the library has in force for a case (context.h band_cdelta,
    band_cdelta_far): what oracle.band_travel is given when no context is there to read them from."""
    o = dict(LIB_DEFAULTS)
    o.update({k: v for k, v in c.opts.items() if k in o})
    if "cdelta" not in c.opts:
        j = jump_density(*model_arrays(c.model, c.nz, c.nx))
        o["cdelta"] = 0.5 if j <= 0.3 else 0.2 if j >= 0.6 else 0.5 + (0.2 - 0.5) * (j - 0.3) / (0.6 - 0.3)
    if o["cdelta_far"] < 0:
        o["cdelta_far"] = 1.4 * o["cdelta"]
    elif o["cdelta_far"] > 0:
        o["cdelta_far"] = max(o["cdelta_far"], o["cdelta"])
    return o


def sources(nz, nx):
    """The 13 source nodes (ix, iz) of a grid: corners, edge midpoints, the columns next to the
    stripe boundaries of 8- and 64-column stripes (top row and interior), one interior node off
    every boundary.  On the 2-row and 3-column grids they are clipped to the grid (some coincide)."""
    cx, cz = nx - 1, nz - 1
    s = [(0, 0), (cx, 0), (0, cz), (cx, cz),
         (nx // 2, 0), (nx // 2, cz), (0, nz // 2), (cx, nz // 2),
         (7, 0), (8, 0), (63, nz // 3), (64, nz // 2 + 3),
         (nx // 3 + 2, (2 * nz) // 3)]
    return [(min(x, cx), min(z, cz)) for x, z in s]


def source_xy(c, src):
    """A source node in metres, as the library and the model take it."""
    return c.gox + c.dnx * src[0], c.goz + c.dnz * src[1]


_fields = {}


def model_field(c, src, opt=None, vmax=None):
    """The CPU band model's field of one source of a case, with the options `opt` and `vmax` read
    back from a context (default: lib_options / vmax_of).  Cached per (model, grid, spacing, origin,
    source, options): the tests that share a configuration share its reference; the arrays are
    read-only."""
    o = lib_options(c) if opt is None else opt
    vmax = model_vmax(c) if vmax is None else vmax
    key = (c.model, c.nz, c.nx, c.dnx, c.dnz, c.gox, c.goz, tuple(src), vmax,
           tuple(float(o[k]) for k in ("cdelta", "cdelta_far", "r_far", "r0", "exact_r")))
    if key not in _fields:
        veln, velpn, vm, sd = model_arrays(c.model, c.nz, c.nx)
        x, z = source_xy(c, src)
        B, _ = O.band_travel(x, z, veln, velpn, vm, sd, TABLE, TABLE, vmax, cdelta=o["cdelta"], exact_init=True,
                             r0=o["r0"], exact_r=o["exact_r"], gox=c.gox, goz=c.goz, dnx=c.dnx, dnz=c.dnz,
                             cdelta_far=o["cdelta_far"], r_far=o["r_far"])
        B.setflags(write=False)
        _fields[key] = B
    return _fields[key]


# ---- the matrix ----
# every model at the default geometry (its own shape, the library's member choice)
MODEL_CASES = [case(m, m) for m in MODELS]
# every shape on the one-record and the grain model.  (Not on the mixed model: on 129 x 97, source
# (63, 43), the CPU band model itself moves by 4.6e-9 between glibc's trigonometric functions and
# the device's correctly rounded ones (oracle/lib/liboracle_cr.so) — a result just over half an ulp
# off flips a stencil choice — and the device follows the latter, so the 1e-9 bar cannot be held
# against the glibc model there; the other 77 mixed fields of the six shapes measured <= 3.8e-16.)
SHAPE_CASES = [case("%s_%dx%d" % (m, nz, nx), m, (nz, nx)) for m in ("iso", "grain") for nz, nx in SHAPES]
# every parameter alone (three sources each: a corner, a stripe-boundary column, the interior)
PARAM_SOURCES = (0, 10, 12)
PARAM_CASES = [
    case("cdelta01", "grain", opts={"cdelta": 0.1}),
    case("exact_r4", "mixed", opts={"exact_r": 4}),
    case("exact_r48", "mixed", opts={"exact_r": 48}),
    case("r0_0", "grain", opts={"r0": 0}),
    case("r0_10", "mixed", opts={"r0": 10}),
    case("dnx2e-4", "grain", dnx=2e-4),
    case("dnz15e-4", "grain", dnx=1e-3, dnz=1.5e-3),
]
# the far band, moved in so that it engages on a 129 x 129 grid: corner source
FAR_CASE = case("far", "grain", (129, 129), opts={"cdelta_far": 0.7, "r_far": 32})
FAR_OFF_CASE = case("far_off", "grain", (129, 129), opts={"cdelta_far": 0.0})
FAR_SOURCE = (0, 0)
# a nonzero origin, and the same case without it
ORIGIN_CASE = case("origin", "grain", gox=0.0125, goz=-0.003)
ORIGIN_ZERO = case("origin_zero", "grain")
# member geometries (stripe_log, members); (0, 0) is what a user gets
MEMBER_GEOMS = [(3, k) for k in range(1, 17)] + [(4, 2), (4, 7), (0, 0)]
MEMBER_CASES = [case(m + "_members", m) for m in ("mixed", "grain")]
# the material paths past the LDS table with several members
MEMBER_CASES_HBM = [case(m + "_members", m) for m in ("many_mid", "many_big")]
# (65 columns are 9 stripes of 8: at most 9 members there)
MEMBER_GEOMS_HBM = {"many_mid": [(3, 1), (3, 2), (3, 5), (3, 9)], "many_big": [(3, 1), (3, 2), (3, 5), (3, 16)]}
# more members asked for than the grid has stripes: (case, stripe_log, members, members in force)
NARROW_CASES = [(case("grain_65x3_narrow", "grain", (65, 3)), 6, 16, 1),
                (case("grain_61x65_narrow", "grain", (61, 65)), 6, 16, 2)]
# streaming out of the kernel (travel_into): ragged last tiles in both directions
STREAM_CASES = [case("grain_stream_97x129", "grain", (97, 129)), case("mixed_stream_41x127", "mixed", (41, 127))]
STREAM_GEOMS = [(3, 1), (3, 3), (3, 16)]


def all_oracle_cases():
    """(case, source) of every model field the GPU test compares with: what the CPU precondition
    test runs."""
    out = []
    for c in MODEL_CASES + SHAPE_CASES + MEMBER_CASES_HBM + [n[0] for n in NARROW_CASES] + STREAM_CASES:
        out += [(c, s) for s in sources(c.nz, c.nx)]
    for c in PARAM_CASES + [ORIGIN_CASE, ORIGIN_ZERO]:
        srcs = sources(c.nz, c.nx)
        out += [(c, srcs[k]) for k in PARAM_SOURCES]
    out += [(FAR_CASE, FAR_SOURCE), (FAR_OFF_CASE, FAR_SOURCE)]
    return out
