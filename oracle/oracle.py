"""ctypes front-end of the CPU oracle (oracle/alifmm_oracle.c).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg as the parity checker.  The product (ali-fmm-and-ray-tracing_amd/) never
imports it.  Every function mirrors the reference function of the same name in
/root/reference/Anis_TTF_rays.py (cited per function) with the reference's argument meaning.
"""
import collections
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ALIFMM_ORACLE_LIB: another build of the same restatement (lib/liboracle_cr.so, the CR-trig one)
_LIB_PATH = os.environ.get("ALIFMM_ORACLE_LIB") or os.path.join(_HERE, "lib", "liboracle.so")
# the two builds of the restatement by name, for open_lib(): glibc trig (golden-pinned) and the
# device's correctly rounded trig
LIB_GLIBC = os.path.join(_HERE, "lib", "liboracle.so")
LIB_CR = os.path.join(_HERE, "lib", "liboracle_cr.so")
_lib = None
_libs = {}

_d = ctypes.c_double
_i = ctypes.c_int
_l = ctypes.c_long
_p = ctypes.c_void_p


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


def open_lib(path):
    """A build of the restatement by its path (LIB_GLIBC, LIB_CR), loaded once per process: several
    builds can be used side by side by passing the result as `lib=` to travel, travel_finer_grid,
    time_between_points, find_ray_walked, band_travel and band_travel_finer.  lib() stays the default one (ALIFMM_ORACLE_LIB, else LIB_GLIBC)."""
    path = os.path.abspath(path)
    if path not in _libs:
        if not os.path.exists(path):
            build()
        L = ctypes.CDLL(path)
        L.oref_travel.restype = _i
        L.oref_travel.argtypes = [_d, _d, _i, _i, _p, _p, _p, _p, _p, _p, _i, _d, _d, _d, _d, _p]
        L.oref_travel_finer_grid.restype = _i
        L.oref_travel_finer_grid.argtypes = [_d, _d, _i, _i, _p, _p, _p, _p, _i, _p, _p, _i, _d, _d, _d, _d, _p]
        L.oref_travel_batch.restype = _i
        L.oref_travel_batch.argtypes = [_i, _p, _p, _i, _i, _p, _p, _p, _p, _i, _p, _p, _i, _d, _d, _d, _d, _p, _i]
        L.oref_time_between_points.restype = _d
        L.oref_time_between_points.argtypes = [_d, _d, _d, _d, _d, _i, _p, _i, _i, _i, _p, _p, _p, _p]
        L.oref_find_ray.restype = _l
        L.oref_find_ray.argtypes = [_d, _p, _i, _d, _d, _d, _d, _p, _i, _i, _i, _i, _p, _p, _p, _p, _i, _p, _p, _l,
                                    _p, _p]
        L.oref_update.restype = _d
        L.oref_update.argtypes = [_i, _i, _p, _p, _i, _i, _d, _i, _i, _p, _p, _p, _p, _p, _i]
        L.oref_fouds18.restype = _d
        L.oref_fouds18.argtypes = [_i, _i, _p, _p, _i, _i, _d, _d, _p, _p, _p, _p, _p, _i]
        L.oref_group_vel.restype = _d
        L.oref_group_vel.argtypes = [_d, _l, _l, _l, _l, _l, _d]
        L.oref_find_ray_walked.restype = _l
        L.oref_find_ray_walked.argtypes = L.oref_find_ray.argtypes + [_p]
        # the band model (band_model.c)
        L.oband_set_far.restype = None
        L.oband_set_far.argtypes = [_d, _d]
        L.oband_travel.restype = _i
        L.oband_travel.argtypes = [_d, _d, _i, _i, _p, _p, _p, _p, _p, _p, _i, _d, _d, _d, _d, _d, _d, _i, _i, _d, _d,
                                   _p, _p]
        L.oband_travel_finer.restype = _i
        L.oband_travel_finer.argtypes = [_d, _d, _i, _i, _p, _p, _p, _p, _p, _p, _i, _i, _d, _d, _d, _d, _d, _d, _d, _d,
                                         _d, _d, _p, _p]
        L.oband_seeded.restype = _i
        L.oband_seeded.argtypes = [_i, _i, _p, _p, _p, _p, _p, _p, _i, _d, _d, _l, _p, _p, _d, _d, _d, _d, _d, _p, _p]
        L.oband_log_begin.restype = None
        L.oband_log_begin.argtypes = [_p, _p, _p, _p, _l]
        L.oband_log_end.restype = _l
        _libs[path] = L
    return _libs[path]


def lib():
    global _lib
    if _lib is None:
        _lib = open_lib(_LIB_PATH)
    return _lib


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _ptr(a):
    return None if a is None else a.ctypes.data


class _Model:
    """Model arrays converted once to the dtypes the oracle reads (int64 velpn / stiffness)."""

    def __init__(self, veln, velpn, vel_map, stif_den, avlist2, phase_vel):
        self.veln = _f64(veln)
        self.velpn = _i64(velpn)
        self.vel_map = _f64(vel_map)
        self.stif = None if stif_den is None else _i64(stif_den)
        self.av = _f64(avlist2)
        self.ph = _f64(phase_vel if phase_vel is not None else avlist2)
        assert self.av.shape == self.ph.shape and self.av.shape[0] == 361
        self.nnz, self.nnx = self.veln.shape
        self.ncol = self.av.shape[1]


def travel(scx, scz, veln, velpn, vel_map, stif_den, avlist2, phase_vel, gox=0.0, goz=0.0, dnx=1e-3, dnz=None,
           lib=None):
    """travel() Anis_TTF_rays.py:1463-2117 (fresh zero ttn; padded stage-1 semantics).
    lib: a build from open_lib() (default: lib())."""
    m = _Model(veln, velpn, vel_map, stif_den, avlist2, phase_vel)
    dnz = dnx if dnz is None else dnz
    out = np.zeros((m.nnz, m.nnx))
    L = lib if lib is not None else globals()["lib"]()
    rc = L.oref_travel(scx, scz, m.nnz, m.nnx, _ptr(m.veln), _ptr(m.velpn), _ptr(m.vel_map), _ptr(m.stif),
                           _ptr(m.av), _ptr(m.ph), m.ncol, gox, goz, dnx, dnz, _ptr(out))
    if rc:
        raise RuntimeError("oracle travel failed rc=%d" % rc)
    return out


def travel_finer_grid(scx, scz, veln, velpn, vel_map, stif_den, subgrid_size, avlist2, phase_vel, gox=0.0, goz=0.0,
                      dnx=1e-3, dnz=None, lib=None):
    """travel_finer_grid() Anis_TTF_rays.py:2120-2832 (returns ttn / subgrid_size).
    lib: a build from open_lib() (default: lib())."""
    m = _Model(veln, velpn, vel_map, stif_den, avlist2, phase_vel)
    dnz = dnx if dnz is None else dnz
    sg = int(subgrid_size)
    out = np.zeros((sg * (m.nnz - 1) + 1, sg * (m.nnx - 1) + 1))
    L = lib if lib is not None else globals()["lib"]()
    rc = L.oref_travel_finer_grid(scx, scz, m.nnz, m.nnx, _ptr(m.veln), _ptr(m.velpn), _ptr(m.vel_map),
                                      _ptr(m.stif), sg, _ptr(m.av), _ptr(m.ph), m.ncol, gox, goz, dnx, dnz,
                                      _ptr(out))
    if rc:
        raise RuntimeError("oracle travel_finer_grid failed rc=%d" % rc)
    return out


def travel_batch(scx, scz, veln, velpn, vel_map, stif_den, avlist2, phase_vel, subgrid_size=1, gox=0.0, goz=0.0,
                 dnx=1e-3, dnz=None, n_threads=1):
    """Many independent sources, one per pthread (the reference's update_parallel :3938, minus its race)."""
    m = _Model(veln, velpn, vel_map, stif_den, avlist2, phase_vel)
    dnz = dnx if dnz is None else dnz
    scx = _f64(scx)
    scz = _f64(scz)
    sg = int(subgrid_size)
    fz, fx = (m.nnz, m.nnx) if sg <= 1 else (sg * (m.nnz - 1) + 1, sg * (m.nnx - 1) + 1)
    out = np.zeros((len(scx), fz, fx))
    rc = lib().oref_travel_batch(len(scx), _ptr(scx), _ptr(scz), m.nnz, m.nnx, _ptr(m.veln), _ptr(m.velpn),
                                 _ptr(m.vel_map), _ptr(m.stif), sg, _ptr(m.av), _ptr(m.ph), m.ncol, gox, goz, dnx,
                                 dnz, _ptr(out), int(n_threads))
    if rc:
        raise RuntimeError("oracle travel_batch failed rc=%d" % rc)
    return out


def time_between_points(x1, x2, y1, y2, dnx, subgrid_size, velocity_dat, veln, velpn, vel_map, stif_den, lib=None):
    """time_between_points() Anis_TTF_rays.py:2835-2989.  lib: a build from open_lib() (default: lib())."""
    m = velocity_dat if isinstance(velocity_dat, _Model) else _Model(veln, velpn, vel_map, stif_den, velocity_dat,
                                                                     velocity_dat)
    L = lib if lib is not None else globals()["lib"]()
    return L.oref_time_between_points(float(x1), float(x2), float(y1), float(y2), dnx, int(subgrid_size),
                                          _ptr(m.av), m.ncol, m.nnz, m.nnx, _ptr(m.veln), _ptr(m.velpn),
                                          _ptr(m.vel_map), _ptr(m.stif))


def find_ray(dnx, velocity_dat, source, receiver, rec_TTF, veln, velpn, vel_map, stif_den, subgrid_size):
    """find_ray() Anis_TTF_rays.py:3104-3465 -> (ray_x, ray_y, trav_time) on the fine grid."""
    m = _Model(veln, velpn, vel_map, stif_den, velocity_dat, velocity_dat)
    ttf = _f64(rec_TTF)
    cap = 5 * (m.nnz + m.nnx)
    rx = np.zeros(cap)
    ry = np.zeros(cap)
    t = ctypes.c_double(0.0)
    early = ctypes.c_int(0)
    n = lib().oref_find_ray(dnx, _ptr(m.av), m.ncol, float(source[0]), float(source[1]), float(receiver[0]),
                            float(receiver[1]), _ptr(ttf), ttf.shape[0], ttf.shape[1], m.nnz, m.nnx, _ptr(m.veln),
                            _ptr(m.velpn), _ptr(m.vel_map), _ptr(m.stif), int(subgrid_size), _ptr(rx), _ptr(ry), cap,
                            ctypes.byref(t), ctypes.byref(early))
    if n < 0:
        raise RuntimeError("oracle find_ray failed rc=%d" % n)
    return rx[:n].copy(), ry[:n].copy(), t.value


def model(velocity_dat, veln, velpn, vel_map, stif_den):
    """The model arrays converted once, for many time_between_points / find_ray_walked calls on one
    model (pass it as `velocity_dat`; the other model arguments are then ignored)."""
    return _Model(veln, velpn, vel_map, stif_den, velocity_dat, velocity_dat)


def find_ray_walked(dnx, velocity_dat, source, receiver, rec_TTF, veln, velpn, vel_map, stif_den, subgrid_size,
                    cap=None, lib=None):
    """find_ray() with everything it returns -> (rc, early, ray_x, ray_y, time, walked).
    rc: the point count, or -3 (the point capacity 5 (nnz + nnx), or `cap` if smaller) or -4 (an
    empty search plane); early: the "travel time to receiver increasing" exit; ray_x / ray_y: the rc
    points, or on a negative rc the `walked` points written before it (time is then 0.0).
    lib: a build from open_lib() (default: lib())."""
    m = velocity_dat if isinstance(velocity_dat, _Model) else _Model(veln, velpn, vel_map, stif_den, velocity_dat,
                                                                     velocity_dat)
    L = lib if lib is not None else globals()["lib"]()
    ttf = _f64(rec_TTF)
    full = 5 * (m.nnz + m.nnx)
    cap = full if cap is None else int(cap)
    rx = np.zeros(max(cap, 2))
    ry = np.zeros(max(cap, 2))
    t = ctypes.c_double(0.0)
    early = ctypes.c_int(0)
    walked = ctypes.c_long(0)
    n = L.oref_find_ray_walked(dnx, _ptr(m.av), m.ncol, float(source[0]), float(source[1]), float(receiver[0]),
                               float(receiver[1]), _ptr(ttf), ttf.shape[0], ttf.shape[1], m.nnz, m.nnx, _ptr(m.veln),
                               _ptr(m.velpn), _ptr(m.vel_map), _ptr(m.stif), int(subgrid_size), _ptr(rx), _ptr(ry),
                               cap, ctypes.byref(t), ctypes.byref(early), ctypes.byref(walked))
    k = n if n >= 0 else walked.value
    return int(n), int(early.value), rx[:k].copy(), ry[:k].copy(), t.value if n >= 0 else 0.0, int(k)


def update(veln, velpn, vel_map, nsts, ttn, iz, ix, dnx, nnz, nnx, phase_vel, stif_den):
    """update() Anis_TTF_rays.py:904-1410 on caller arrays (nnz/nnx are the reference arguments)."""
    ttn = _f64(ttn)
    nsts = np.ascontiguousarray(nsts, dtype=np.int32)
    m = _Model(veln, velpn, vel_map, stif_den, phase_vel, phase_vel)
    return lib().oref_update(ttn.shape[0], ttn.shape[1], _ptr(ttn), _ptr(nsts), int(iz), int(ix), dnx, int(nnz),
                             int(nnx), _ptr(m.veln), _ptr(m.velpn), _ptr(m.vel_map), _ptr(m.stif), _ptr(m.ph), m.ncol)


def fouds18_A(iz, ix, nsts, ttn, dnx, dnz, nnx, nnz, veln, velpn, vel_map, avlist2, stif_den):
    """fouds18_A() Anis_TTF_rays.py:240-901 on caller arrays."""
    ttn = _f64(ttn)
    nsts = np.ascontiguousarray(nsts, dtype=np.int32)
    assert ttn.shape == (nnz, nnx)
    m = _Model(veln, velpn, vel_map, stif_den, avlist2, avlist2)
    return lib().oref_fouds18(int(nnz), int(nnx), _ptr(ttn), _ptr(nsts), int(iz), int(ix), dnx, dnz, _ptr(m.veln),
                              _ptr(m.velpn), _ptr(m.vel_map), _ptr(m.stif), _ptr(m.av), m.ncol)


def group_vel(angle, c_22, c_23, c_33, c_44, sigma, vel_scale=1):
    """group_vel() Anis_TTF_rays.py:3521-3558."""
    return lib().oref_group_vel(float(angle), int(c_22), int(c_23), int(c_33), int(c_44), int(sigma),
                                float(vel_scale))


def band_travel(scx, scz, veln, velpn, vel_map, stif_den, avlist2, phase_vel, vmax, cdelta=0.25, exact_init=False,
                sweeps=1, r0=0.0, exact_r=0.0, gox=0.0, goz=0.0, dnx=1e-3, dnz=None, cdelta_far=0.0, r_far=0.0,
                lib=None):
    """CPU model of the MI355X band-synchronous formulation (oracle/band_model.c). Returns (T, steps[4]).
    cdelta_far / r_far: the device's optional wider band far from the source (0: off).
    lib: a build from open_lib() (default: lib())."""
    m = _Model(veln, velpn, vel_map, stif_den, avlist2, phase_vel)
    dnz = dnx if dnz is None else dnz
    out = np.zeros((m.nnz, m.nnx))
    steps = np.zeros(4, dtype=np.int64)
    L = lib if lib is not None else globals()["lib"]()
    L.oband_set_far(float(cdelta_far), float(r_far))
    rc = L.oband_travel(scx, scz, m.nnz, m.nnx, _ptr(m.veln), _ptr(m.velpn), _ptr(m.vel_map), _ptr(m.stif),
                        _ptr(m.av), _ptr(m.ph), m.ncol, gox, goz, dnx, dnz, cdelta, vmax, int(exact_init),
                        int(sweeps), float(r0), float(exact_r), _ptr(out), _ptr(steps))
    if rc:
        raise RuntimeError("band model failed rc=%d" % rc)
    return out, steps


BandLog = collections.namedtuple("BandLog", "acc cell step flag")


def band_logged(run, ncells, lib=None, per_cell=8):
    """run() (a band_travel or band_seeded call on the same `lib`) with the main grid's band run
    recorded (oracle/band_model.c oband_log_begin) -> (run's result, BandLog): acc[cell] the step
    at which the cell was accepted (-1: never, or known at the hand-over); one entry per close-list
    insertion and evaluation: cell, step (-1: the hand-over) and flag (bit 0: the cell was far and
    joins the close list, bit 1: update() returned -1 and fouds18_A() ran)."""
    L = lib if lib is not None else globals()["lib"]()
    cap = int(per_cell) * int(ncells) + 1024
    acc = np.full(ncells, -1, dtype=np.int32)
    cell, step, flag = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int8)
    L.oband_log_begin(_ptr(acc), _ptr(cell), _ptr(step), _ptr(flag), cap)
    try:
        out = run()
    finally:
        n = L.oband_log_end()
    if n < 0:
        raise RuntimeError("band log: more than %d entries" % cap)
    return out, BandLog(acc, cell[:n].copy(), step[:n].copy(), flag[:n].copy())


def band_seeded(model, seed_cell, seed_t, dnx, dnz, vmax, cdelta, r0, cdelta_far=0.0, r_far=0.0, lib=None):
    """alifmm_travel_seeded as tests/seed_ref.py states it, in C (oracle/band_model.c oband_seeded):
    `model` from model(), seed_cell flat cell indices, the widths in force.  Returns (T, steps)."""
    m = model
    cells, t = np.ascontiguousarray(seed_cell, dtype=np.int32), _f64(seed_t)
    assert cells.shape == t.shape and cells.ndim == 1
    out = np.zeros((m.nnz, m.nnx))
    steps = ctypes.c_long(0)
    L = lib if lib is not None else globals()["lib"]()
    rc = L.oband_seeded(m.nnz, m.nnx, _ptr(m.veln), _ptr(m.velpn), _ptr(m.vel_map), _ptr(m.stif), _ptr(m.av),
                        _ptr(m.ph), m.ncol, float(dnx), float(dnz), len(cells), _ptr(cells), _ptr(t), float(cdelta),
                        float(vmax), float(r0), float(cdelta_far), float(r_far), _ptr(out), ctypes.byref(steps))
    if rc:
        raise RuntimeError("band model (seeded) failed rc=%d" % rc)
    return out, int(steps.value)


FinerInfo = collections.namedtuple("FinerInfo", "steps pops close peak1 peak2 peakp")


def band_travel_finer(scx, scz, veln, velpn, vel_map, stif_den, subgrid_size, avlist2, phase_vel, vmax, cdelta=0.5,
                      r0=40.0, exact_r=20, cdelta_far=0.0, r_far=0.0, gox=0.0, goz=0.0, dnx=1e-3, dnz=None, lib=None):
    """CPU model of the device's travel_finer_grid (oracle/band_model.c oband_travel_finer): the
    reference's two heap stages and the heap-ordered prefix out to (size2 + exact_r) fine nodes, the
    band on the fine view from there, / subgrid_size.  cdelta / cdelta_far are the widths in force
    (the caller applies band_cdelta(ctx, sg) and the far_sg rule).  Returns (T, FinerInfo): band
    steps, nodes the prefix popped, close nodes handed to the band, peak heap entries of stage 1,
    stage 2 and the prefix.  lib: a build from open_lib() (default: lib())."""
    m = _Model(veln, velpn, vel_map, stif_den, avlist2, phase_vel)
    dnz = dnx if dnz is None else dnz
    sg = int(subgrid_size)
    out = np.zeros((sg * (m.nnz - 1) + 1, sg * (m.nnx - 1) + 1))
    info = np.zeros(6, dtype=np.int64)
    L = lib if lib is not None else globals()["lib"]()
    rc = L.oband_travel_finer(scx, scz, m.nnz, m.nnx, _ptr(m.veln), _ptr(m.velpn), _ptr(m.vel_map), _ptr(m.stif),
                              _ptr(m.av), _ptr(m.ph), m.ncol, sg, gox, goz, dnx, dnz, float(cdelta), float(vmax),
                              float(r0), float(exact_r), float(cdelta_far), float(r_far), _ptr(out), _ptr(info))
    if rc:
        raise RuntimeError("band model (finer grid) failed rc=%d" % rc)
    return out, FinerInfo(*[int(v) for v in info])
