"""The case matrix of alifmm_travel_seeded, shared by tests/test_seed_ref.py (the CPU side: every
reference field is finite and positive off its zero-time seeds) and tests/test_gpu_seeded.py (the
device against tests/seed_ref.py).  Models and grids from tests/band_cases.py; every seed set on
every model.  Deterministic.
"""
import collections
import math

import numpy as np

import band_cases as BC
import seed_ref

# iso and mixed on 41 x 127 (the last 8-, 16- and 64-column stripe one column short), grain and
# many_mid on 61 x 65 (column 64 is the last one, a stripe of one column)
MODEL_GRIDS = (("iso", 41, 127), ("mixed", 41, 127), ("grain", 61, 65), ("many_mid", 61, 65))
DNX = 1e-3
# the point source whose field gives the bottom row its times (node ix, iz)
INCIDENT = lambda nz, nx: (nx // 3, 0)  # noqa: E731

SeedSet = collections.namedtuple("SeedSet", "name iz ix t")  # t None: read from the incident field


def case(model, nz, nx):
    return BC.case("seed_%s_%dx%d" % (model, nz, nx), model, (nz, nx), dnx=DNX)


def seed_sets(nz, nx, vmax, dnx=DNX, dnz=DNX):
    z0, xs, zs = np.zeros(nx, dtype=np.int32), np.arange(nx, dtype=np.int32), np.arange(nz, dtype=np.int32)
    k = np.arange(min(nz, nx - 1), dtype=np.int32)
    third = xs[::3]
    zero = lambda a: np.zeros(len(a))  # noqa: E731
    sets = [
        SeedSet("top0", z0, xs, zero(xs)),  # all ties; +0 known on every stripe-edge column
        SeedSet("bottom_from", z0 + (nz - 1), xs, None),
        SeedSet("steer20", z0 + nz // 2, xs, xs * dnx * math.sin(math.radians(20.0)) / vmax),
        SeedSet("two_layers", np.concatenate([z0, z0 + 1]), np.concatenate([xs, xs]),
                np.concatenate([zero(xs), zero(xs) + dnz / vmax])),
        SeedSet("corner", np.array([0], dtype=np.int32), np.array([0], dtype=np.int32), np.zeros(1)),
        SeedSet("node63", np.array([nz // 2], dtype=np.int32), np.array([63], dtype=np.int32), np.zeros(1)),
        SeedSet("node64", np.array([nz // 2], dtype=np.int32), np.array([64], dtype=np.int32), np.zeros(1)),
        SeedSet("column63", zs, 0 * zs + 63, zero(zs)),
        SeedSet("column64", zs, 0 * zs + 64, zero(zs)),
        SeedSet("stairs", np.concatenate([k, k]), np.concatenate([k, k + 1]), zero(np.concatenate([k, k]))),
        SeedSet("every_third", 0 * third + nz // 3, third, zero(third)),
    ]
    return sets


def checkerboard(nz, nx, vmax, dnx=DNX, dnz=DNX):
    """Every second node: every cell of the grid is handed over (seed or close)."""
    zz, xx = np.mgrid[0:nz, 0:nx]
    m = (zz + xx) % 2 == 0
    iz, ix = zz[m].astype(np.int32), xx[m].astype(np.int32)
    return SeedSet("checkerboard", iz, ix, np.hypot(iz * dnz, ix * dnx) / vmax)


CHECKER_FITS = ("grain", 97, 122)   # 5 917 seeds + 5 917 close cells = 11 834 entries
CHECKER_OVER = ("grain", 97, 129)   # 12 513 entries: past the hand-over's 11 881
FAR_GRID = ("grain", 97, 129)
FAR_OPTS = {"cdelta_far": 0.7, "r_far": 20}

_refs = {}
_fields = {}


def ref_for(c):
    k = (c.model, c.nz, c.nx, c.dnx, c.dnz)
    if k not in _refs:
        _refs[k] = seed_ref.SeedRef(*BC.model_arrays(c.model, c.nz, c.nx), BC.TABLE, c.dnx, c.dnz)
    return _refs[k]


def ref_field(c, s, t, opt, vmax):
    """The reference field of seed set s with times t on case c under the band options opt; computed
    once per (case, set, times, options), read-only."""
    t = np.ascontiguousarray(t, dtype=np.float64)
    key = (c.model, c.nz, c.nx, c.dnx, c.dnz, s.name, t.tobytes(), vmax,
           tuple(float(opt[k]) for k in ("cdelta", "r0", "cdelta_far", "r_far")))
    if key not in _fields:
        F = ref_for(c).field(s.iz, s.ix, t, vmax, opt["cdelta"], opt["r0"], opt["cdelta_far"], opt["r_far"])
        F.setflags(write=False)
        _fields[key] = F
    return _fields[key]


def incident_times(c, s, field):
    return np.ascontiguousarray(field[s.iz, s.ix])
