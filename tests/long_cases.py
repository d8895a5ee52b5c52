"""The long-list cases of the band kernel (fmm_band_k.hip) and the list census that chose them,
shared by tests/test_long_cases_ref.py (the CPU side: every reference field is finite, every case
reaches the side of the switch it is named for) and tests/test_gpu_band_long.py (the device against
the CPU models over every cell, and its own list sums against the census).

The kernel keeps the head of each per-step list in LDS and spills the rest; its path changes with
the list lengths (the constants below restate fmm_band_k.hip's; a change there that is not made
here fails the device's own sums against the census).  A point source needs about 1200^2 nodes
before one member's close set passes the LDS head; a plane front seeded on a full row of a 6 x nx
grid has nx cells in every list, and one seeded on a full column of an nz x 24 grid with 8-column
stripes has nz accepted edge cells, nz rim items and nz boundary claims per step.

census(): the CPU band model's record of a run (oracle.band_logged: the step each cell was accepted
in, every close-list insertion and evaluation) counted per band step and member under the ownership
rule of band_common.h KGeom, restated here: stripe s = x >> wlog belongs to member s % K; EDGE cells
lie within 2 columns of a stripe boundary, RIM cells next to one (K > 1).  Deterministic.
"""
import collections

import numpy as np

import band_cases as BC
import oracle as O
import seed_ref
import workloads as W

# fmm_band_k.hip
K_THREADS, K_LCAP, K_ACAP, K_ECAP, K_BCAP, K_DCAP, K_RCAP = 768, 3328, 1536, 1792, 512, 256, 1024
K_SORT_ACC, K_SORT_KMAX, K_FB_ROUND = 256, 8, 128
TS_LIST_CAP, TS_OWN_TILE_MAX = 32, 1024  # tile_stream.h
HANDOVER_MAX = 11881
DNX = 1e-3

Census = collections.namedtuple(
    "Census", "steps K wlog close hi accepted acc_edge rim rim_read rx items ei eb fresh fallback nf_end tiles")
Census.__doc__ = """Per band step (rows 0 .. steps - 1) and member (columns), what fmm_band_k.hip holds:
close: live close cells before the accept; hi: the close set's high-water mark before the accept (the
slots scanned; hi <= kLcap keeps it in LDS); accepted; acc_edge: accepted EDGE cells (the Dc list);
rim: live RIM cells published in P1; rim_read: entries of the neighbour members' rim lists read back;
rx: claim items received (accepted RIM cells of the neighbours whose cross neighbour is own);
items: 4 accepted + rx; ei / eb: interior / boundary (EDGE) claims; fresh: claims of far cells (new
close-set slots); fallback: cells for which update() returned -1; nf_end: free slots after the commit;
tiles: own W x 2^trlog tiles whose last cell became known (None without trlog; row 0 includes the
tiles complete at the hand-over)."""


def stream_trlog(K, wlog, nz, nx):
    """tile_stream.h plan(): the fewest tile rows 2^trlog that keep a member's own tiles within 1024."""
    own = (((nx + (1 << wlog) - 1) >> wlog) + K - 1) // K
    trlog = 2
    while trlog < 14 and own * ((nz + (1 << trlog) - 1) >> trlog) > TS_OWN_TILE_MAX:
        trlog += 1
    return trlog


def wlog_for(K, stripe_log):
    """host_travel.cpp travel_chunk: the stripe width follows the member count unless stripe_log fixes it."""
    return stripe_log if stripe_log else (4 if K >= 16 else 5 if K >= 8 else 6)


def census(log, nz, nx, K, wlog, trlog=None):
    Wm = (1 << wlog) - 1
    multi = K > 1

    def geom(cell):
        x = cell.astype(np.int64) % nx
        r = x & Wm
        own = (x >> wlog) % K
        edge = multi & ((r < 2) | (r >= Wm - 1))
        rim = multi & (((r == 0) & (x > 0)) | ((r == Wm) & (x < nx - 1)))
        return x, r, own, edge, rim

    steps = int(log.acc.max()) + 1
    assert steps > 0 and (len(log.step) == 0 or int(log.step.max()) < steps)

    def count(step, own, mask=None):  # row 0: step -1
        k = (step.astype(np.int64) + 1) * K + own
        if mask is not None:
            k = k[mask]
        return np.bincount(k, minlength=(steps + 1) * K).reshape(steps + 1, K)

    ac = np.nonzero(log.acc >= 0)[0]
    ast = log.acc[ac]
    ax, ar, aown, aedge, arim = geom(ac)
    accepted = count(ast, aown)
    acc_edge = count(ast, aown, aedge)
    acc_rim = count(ast, aown, arim)
    # claim items: the cross-boundary neighbour of an accepted RIM cell, counted for its owner
    cx = np.where(ar == 0, ax - 1, ax + 1)
    rx = count(ast, (np.clip(cx, 0, nx - 1) >> wlog) % K, arim)
    ex, er, eown, eedge, erim = geom(log.cell)
    far, band = (log.flag & 1) != 0, log.step >= 0
    fresh = count(log.step, eown, far)
    fresh_rim = count(log.step, eown, far & erim)
    ei = count(log.step, eown, band & ~eedge)
    eb = count(log.step, eown, band & eedge)
    fallback = count(log.step, eown, band & ((log.flag & 2) != 0))

    def live(ins, out):  # before the accept of step s: inserted in steps -1 .. s - 1, accepted in 0 .. s - 1
        return (np.cumsum(ins, 0)[:-1] - np.cumsum(out, 0)[:-1])

    close, rim = live(fresh, accepted), live(fresh_rim, acc_rim)
    if K == 1:
        rim_read = np.zeros_like(rim)
    elif K == 2:
        rim_read = rim[:, ::-1].copy()
    else:
        rim_read = np.roll(rim, 1, 1) + np.roll(rim, -1, 1)
    accepted, acc_edge, rx, ei, eb, fallback = (a[1:] for a in (accepted, acc_edge, rx, ei, eb, fallback))
    # the close set's slots: accepted slots are freed (nF), fresh cells take freed slots first, then
    # new ones past the high-water mark (the commit, P5)
    hi, nf_end = np.zeros((steps, K), dtype=np.int64), np.zeros((steps, K), dtype=np.int64)
    h, nf = fresh[0].astype(np.int64), np.zeros(K, dtype=np.int64)
    for s in range(steps):
        hi[s] = h
        nf = nf + accepted[s]
        taken = fresh[s + 1]
        h = h + np.maximum(0, taken - nf)
        nf = np.maximum(0, nf - taken)
        nf_end[s] = nf
    assert np.array_equal(hi - np.vstack([np.zeros((1, K), dtype=np.int64), nf_end[:-1]]), close)
    tiles = None
    if trlog is not None:
        known = log.acc.reshape(nz, nx).astype(np.int64)
        ntz, nstr = (nz + (1 << trlog) - 1) >> trlog, (nx + Wm) >> wlog
        done = np.full((ntz, nstr), -1, dtype=np.int64)
        zz, xx = np.mgrid[0:nz, 0:nx]
        np.maximum.at(done, (zz >> trlog, xx >> wlog), known)
        town = np.broadcast_to(np.arange(nstr) % K, done.shape)
        tiles = np.bincount((np.maximum(done, 0) * K + town).ravel(), minlength=steps * K).reshape(steps, K)
    return Census(steps, K, wlog, close, hi, accepted, acc_edge, rim, rim_read, rx, 4 * accepted + rx, ei, eb,
                  fresh[1:], fallback, nf_end, tiles)


def device_sums(c, member=0):
    """alifmm_band_profile entries 6 .. 9 of a run with option prof 1 (the kernel's ls[0 .. 2] and
    lmax, kept by `member` 0): the sums over the steps of hi minus the free slots after the commit,
    of the accepted and of the evaluated cells, and the largest hi."""
    m = member
    return (int((c.hi[:, m] - c.nf_end[:, m]).sum()), int(c.accepted[:, m].sum()), int((c.ei + c.eb)[:, m].sum()),
            int(c.hi[:, m].max()))


# ---- the switches of the kernel's step: (what is compared, the constant it is compared with) ----
SWITCHES = {
    "close_lds": (lambda c: c.hi, K_LCAP),                 # hi <= kLcap: close set in LDS
    "accepted_lds": (lambda c: c.accepted, K_ACAP),        # nA <= kAcap: accepted list (and claim items) in LDS
    "sort": (lambda c: c.accepted, K_SORT_ACC),            # nA > kSortAcc (and <= kAcap, K <= kSortKmax): counting sort
    "single_pass": (lambda c: c.items, K_THREADS),         # 4 nA + nRx <= kThreads: one claim pass
    "rx_lds": (lambda c: c.rx, K_RCAP),                    # nRx <= kRcap: claim items in LDS
    "eval_lds": (lambda c: c.ei + c.eb, K_ECAP),           # nE <= kEcap: evaluation in LDS
    "bnd_lds": (lambda c: c.eb, K_BCAP),                   # nEb <= kBcap: ... and its boundary list
    "commit_lds": (lambda c: c.hi + c.ei + c.eb, K_LCAP),  # hi + nE <= kLcap: LDS commit
    "edge_lds": (lambda c: c.acc_edge, K_DCAP),            # accepted edge cells per step parity
    "rim_prefetch": (lambda c: c.rim_read, K_THREADS),     # rim entries read back: the prefetched kThreads, then a loop
    "fb_round": (lambda c: c.fallback, K_FB_ROUND),        # fouds18_A() fallback: staging rounds of kFbRound cells
    "fb_list": (lambda c: c.fallback, K_RCAP),             # ... listed up to kRcap, found by a scan past it
}
WINDOW = 64


def side_reached(c, switch, side):
    """The largest per-step, per-member value of a switch's quantity lies in (cap - 64, cap] ("under")
    or in (cap, cap + 64] ("over"); returns (holds, value)."""
    f, cap = SWITCHES[switch]
    v = int(f(c).max())
    return (cap - WINDOW < v <= cap) if side == "under" else (cap < v <= cap + WINDOW), v


# kind: "row" (seeds: row 0, every column), "col" (seeds: every row of column arg), "thirds" (every
# third row, column arg), "travel" (a point source (ix, iz)).  geoms: (stripe_log, members) run beside
# the one-member run.  reach: (switch, side, members) the census must show.
LongCase = collections.namedtuple("LongCase", "name kind model nz nx arg geoms reach")


def _h(nx, reach, geoms=()):
    return LongCase("h_6x%d" % nx, "row", "iso", 6, nx, None, tuple(geoms), tuple((s, d, 1) for s, d in reach))


H_CASES = [
    _h(192, [("single_pass", "under")]),
    _h(200, [("single_pass", "over")]),
    _h(256, [("sort", "under")]),
    _h(300, [("sort", "over")]),
    _h(1536, [("accepted_lds", "under")]),
    _h(1570, [("accepted_lds", "over")]),
    _h(1664, [("commit_lds", "under")]),
    _h(1680, [("commit_lds", "over")]),
    _h(1792, [("eval_lds", "under")]),
    _h(1820, [("eval_lds", "over")]),
    _h(3328, [("close_lds", "under")]),
    _h(3360, [("close_lds", "over")]),
    # every list past its head at one member; per member 1700 (past kAcap), 850 and 425 (sorted), 212
    _h(3400, [], geoms=[(0, 2), (0, 4), (0, 8), (0, 16)]),
    # 625 accepted cells per member at 8 members (sorted), 312 at 16 (past kSortAcc, not sorted:
    # kSortKmax); 5000 seeds + 5000 close cells of the hand-over's 11 881
    _h(5000, [], geoms=[(0, 8), (0, 16)]),
]
# the accepted-list lengths (low, high] the multi-member H runs must show: (case, members, sorted)
SORT_WINDOWS = [("h_6x3400", 4, True), ("h_6x3400", 8, True), ("h_6x5000", 8, True), ("h_6x5000", 16, False)]


def _v(nz, reach, nx=24):
    return LongCase("v_%dx%d" % (nz, nx), "col", "iso", nz, nx, 0, ((3, 2), (3, 3)),
                    tuple((s, d, k) for s, d in reach for k in (2, 3)))


V_CASES = [
    _v(256, [("edge_lds", "under")]),
    _v(300, [("edge_lds", "over")]),
    _v(512, [("bnd_lds", "under")]),
    _v(560, [("bnd_lds", "over")]),
    _v(768, [("rim_prefetch", "under")]),
    _v(800, [("rim_prefetch", "over")]),
    _v(1024, [("rx_lds", "under")]),
    _v(1060, [("rx_lds", "over")]),
    _v(800, [("rim_prefetch", "over")], nx=25),  # a last stripe of one column (member 0's at 3 members)
]



def _f(n, reach):
    return LongCase("f_%dx24" % (3 * n), "thirds", "iso", 3 * n, 24, 10, ((3, 2), (3, 3)),
                    tuple((s, d, k) for s, d in reach for k in (1, 2, 3)))


# n zero-time seeds in every third row of column 10: step 0 accepts all their close cells and claims,
# among others, the cells two columns from each seed (columns 8 and 12), for which update() has no
# usable stencil: 2 n + 1 fallback cells in one step, those of column 8 (the first of member 1's
# stripe) with windows that reach into member 0's columns
F_CASES = [
    _f(60, [("fb_round", "under")]),
    _f(70, [("fb_round", "over")]),
    _f(500, [("fb_list", "under")]),
    _f(520, [("fb_list", "over")]),
]

RAGGED_N = 1200
RAGGED_CASES = [LongCase("ragged_%s" % n, "travel", "grain1200", RAGGED_N, RAGGED_N, src, ((0, 2),), ())
                for n, src in (("centre", (600, 600)), ("corner", (0, 0)), ("edge", (600, 0)))]
# census only (the fallback and the streaming counts): no device run
MIXED_CENSUS_CASE = LongCase("mixed_600_centre", "travel", "mixed", 600, 600, (300, 300), ((0, 2),), ())

# capacity: 16 members of 8-column stripes on 128 columns.  The work lists hold max(65536, cells / 8)
# entries per source (host_travel.cpp travel_chunk), a 16th of it per member: 4096 on both grids.
# loud: a full column of seeds at column 3 hands member 0 the 7800 close cells of columns 2 and 4.
# (3900 rows, not more: 3 x 3900 = 11 700 seeds and close cells of the hand-over's 11 881.)
CAP_LOUD = LongCase("cap_loud_3900x128", "col", "iso", 3900, 128, 3, ((3, 16),), ())
# dropped claims: 1000 seeds in every third row of column 2; member 0's 3999 close cells are all
# accepted in step 0, which claims 3000 interior cells (columns 3, 4) and 2999 boundary cells
# (columns 0, 1): each list within 4096, their sum not
CAP_DROPPED = LongCase("cap_dropped_3000x128", "thirds", "iso", 3000, 128, 2, ((3, 16),), ())
CAP_PER_MEMBER = 4096

ALL_DEVICE_CASES = H_CASES + V_CASES + F_CASES + RAGGED_CASES + [CAP_LOUD, CAP_DROPPED]

# what the census found on the point-source cases (the ragged ones and the mixed one, one and two
# members; tests/test_long_cases_ref.py holds them): the most fallback cells of one member in one
# step (the F cases are there for the fallback's rounds and its scan) and the most tiles one member
# completes in one step (ts::kListCap 32 per step: no case reaches a second list)
FALLBACK_MOST, TILES_MOST = 1, 6


def seeds_of(c):
    """(iz, ix, t) of a seeded case: zero-time seeds."""
    if c.kind == "row":
        iz, ix = np.zeros(c.nx, dtype=np.int32), np.arange(c.nx, dtype=np.int32)
    elif c.kind == "col":
        iz, ix = np.arange(c.nz, dtype=np.int32), np.full(c.nz, c.arg, dtype=np.int32)
    elif c.kind == "thirds":
        iz = np.arange(0, c.nz, 3, dtype=np.int32)
        ix = np.full(len(iz), c.arg, dtype=np.int32)
    else:
        raise KeyError(c.kind)
    return iz, ix, np.zeros(len(iz))


_models = {}


def model_arrays(c):
    """(veln, velpn, vel_map, stif_den); "grain1200": the grains of the 401^2 band-model tests at 1200^2."""
    if c.model != "grain1200":
        return BC.model_arrays(c.model, c.nz, c.nx)
    if c.model not in _models:
        n = RAGGED_N
        m = (W.voronoi_small(n, seed=5), np.zeros((n, n), dtype=np.int64), np.ones((n, n)), W.stif_field(n, n))
        for a in m:
            a.setflags(write=False)
        _models[c.model] = m
    return _models[c.model]


_opts = {}


def lib_options(c):
    """(band options, vmax) the library has in force for a case (as band_cases.lib_options, vmax_of)."""
    k = (c.model, c.nz, c.nx)
    if k not in _opts:
        veln, velpn, vm, sd = model_arrays(c)
        o = dict(BC.LIB_DEFAULTS)
        j = BC.jump_density(veln, velpn, vm, sd)
        o["cdelta"] = 0.5 if j <= 0.3 else 0.2 if j >= 0.6 else 0.5 + (0.2 - 0.5) * (j - 0.3) / (0.6 - 0.3)
        o["cdelta_far"] = 1.4 * o["cdelta"]
        if c.model == "grain1200":  # one material record but for the orientation: one cell gives the speed
            vmax = BC.vmax_of(velpn[:1, :1], vm[:1, :1], sd[:1, :1], BC.TABLE)
        else:
            vmax = BC.vmax_of(velpn, vm, sd, BC.TABLE)
        _opts[k] = (o, vmax)
    return _opts[k]


def cr_lib():
    """The CPU models with the device's correctly rounded trigonometric functions."""
    return O.open_lib(O.LIB_CR)


_refs = {}


def reference(c, opt=None, vmax=None):
    """(field, oracle.BandLog) of a case by the CPU model (tests/seed_ref.py SeedRef.field_c for the
    seeded kinds, oracle.band_travel for "travel"; the correctly rounded build), under the band
    options and vmax read back from a context (default: lib_options).  Computed once per (case,
    options), read-only."""
    o, v = lib_options(c) if opt is None or vmax is None else (opt, vmax)
    o = dict(BC.LIB_DEFAULTS, **o)
    key = (c.name, v, tuple(float(o[k]) for k in ("cdelta", "cdelta_far", "r_far", "r0", "exact_r")))
    if key not in _refs:
        veln, velpn, vm, sd = model_arrays(c)
        if c.kind == "travel":
            run = lambda: O.band_travel(DNX * c.arg[0], DNX * c.arg[1], veln, velpn, vm, sd, BC.TABLE, BC.TABLE, v,  # noqa: E731
                                        cdelta=o["cdelta"], exact_init=True, r0=o["r0"], exact_r=o["exact_r"], dnx=DNX,
                                        cdelta_far=o["cdelta_far"], r_far=o["r_far"], lib=cr_lib())[0]
            F, log = O.band_logged(run, c.nz * c.nx, lib=cr_lib())
        else:
            iz, ix, t = seeds_of(c)
            R = seed_ref.SeedRef(veln, velpn, vm, sd, BC.TABLE, DNX)
            F, log = R.field_c(iz, ix, t, v, o["cdelta"], o["r0"], o["cdelta_far"], o["r_far"], lib=cr_lib(), log=True)
        for a in (F,) + tuple(log):
            a.setflags(write=False)
        _refs[key] = (F, log)
    return _refs[key]


def census_of(c, members, stripe_log, opt=None, vmax=None, tiles=False):
    wlog = wlog_for(members, stripe_log)
    trlog = stream_trlog(members, wlog, c.nz, c.nx) if tiles else None
    return census(reference(c, opt, vmax)[1], c.nz, c.nx, members, wlog, trlog)


def same_lists(a, b):
    """Two censuses hold the same counts in every step and member."""
    return a.steps == b.steps and all(np.array_equal(x, y) for x, y in zip(a[3:], b[3:]) if x is not None)


def tied_to_cpu(c, opt, vmax, geoms):
    """What a context has in force for case c (band options, vmax) is what tests/test_long_cases_ref.py
    checked the case under: the same options, vmax to the last bits (the context's own arithmetic), and
    the same lists in every step under every member geometry (stripe_log, members)."""
    o, v = lib_options(c)
    if any(float(opt[k]) != float(o[k]) for k in o) or abs(vmax - v) > 1e-12 * v:
        return False
    return all(same_lists(census_of(c, k, sl, opt, vmax), census_of(c, k, sl)) for sl, k in geoms)
