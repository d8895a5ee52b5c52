"""ctypes binding of libalifmm.so (include/alifmm.h) — the MI355X hot path.

The library is built in-tree (csrc/Makefile -> lib/libalifmm.so).  There is no CPU fallback:
if the library or a GPU is missing, every entry point raises AlifmmError.
"""
import atexit
import ctypes
import os
import threading
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ALIFMM_LIB") or os.path.join(HERE, "lib", "libalifmm.so")  # override: experiments

_d, _i, _l, _p = ctypes.c_double, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
_lib = None
_lib_closed = False
_lock = threading.Lock()
_live = weakref.WeakSet()  # open Contexts (shutdown() destroys them)


class AlifmmError(RuntimeError):
    pass


class RayCapacityError(AlifmmError, IndexError):
    """A ray reached the reference's point capacity 5 (nnz + nnx): the reference writes past its
    ray arrays there and raises IndexError (Anis_TTF_rays.py:4287, :3440-3442)."""


# ray flags (kernels.h RayParams::flags)
RAY_EARLY_EXIT, RAY_CAPACITY, RAY_BAD_PLANE = 1, 2, 4
RAY_NO_HIT = 8  # alifmm_skip_rays: no reflector node with a finite time sum (the ray is empty)


def check_ray_flags(flags):
    """Raise for rays the kernel stopped short of the receiver (capacity, empty search plane);
    bit 0 (the reference's "Travel time to receiver increasing" early exit) is normal output."""
    flags = np.asarray(flags)
    bad = np.nonzero(flags & RAY_CAPACITY)[0]
    if len(bad):
        raise RayCapacityError("ray %d reached the point capacity 5 (nnz + nnx)" % int(bad[0]))
    bad = np.nonzero(flags & RAY_BAD_PLANE)[0]
    if len(bad):
        raise AlifmmError("ray %d: empty plane-search candidate set" % int(bad[0]))


def _load():
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if _lib_closed:
            raise AlifmmError("libalifmm.so was unloaded by shutdown() (interpreter exit)")
        if not os.path.exists(LIB_PATH):
            raise AlifmmError("libalifmm.so not built (%s); run `make -C %s/csrc` or __graft_entry__.build()"
                              % (LIB_PATH, HERE))
        L = ctypes.CDLL(LIB_PATH)
        sig = {
            "alifmm_version": (ctypes.c_char_p, []),
            "alifmm_device_count": (_i, [_p]),
            "alifmm_ctx_create": (_i, [_i, _p]),
            "alifmm_ctx_destroy": (_i, [_p]),
            "alifmm_last_error": (ctypes.c_char_p, [_p]),
            "alifmm_set_model": (_i, [_p, _i, _i, _p, _p, _p, _p, _p, _p, _i, _d, _d, _d, _d]),
            "alifmm_set_option": (_i, [_p, ctypes.c_char_p, _d]),
            "alifmm_get_option": (_i, [_p, ctypes.c_char_p, _p]),
            "alifmm_field_shape": (_i, [_p, _i, _p, _p]),
            "alifmm_travel": (_i, [_p, _i, _i, _p, _p, _i, _p]),
            "alifmm_travel_into": (_i, [_p, _i, _i, _p, _p, _i, _p]),
            "alifmm_travel_seeded": (_i, [_p, _i, _i, _p, _p, _p, _p, _i, _p]),
            "alifmm_get_field": (_i, [_p, _i, _p]),
            "alifmm_release_fields": (_i, [_p]),
            "alifmm_copy_fields": (_i, [_p, _i, _i, _p, _i, _p]),
            "alifmm_find_rays": (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _p, _l]),
            "alifmm_take_rays": (_i, [_p, _p, _l, _p]),
            "alifmm_skip_pick": (_i, [_p, _i, _p, _p, _i, _p, _p, _p, _p]),
            "alifmm_skip_rays": (_i, [_p, _i, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _l]),
            "alifmm_source_stats": (_i, [_p, _i, _p, _p]),
            "alifmm_last_timing": (_i, [_p, _p, _p, _p]),
            "alifmm_band_profile": (_i, [_p, _i, _p]),
            "alifmm_band_span": (_i, [_p, _i, _p]),
            "alifmm_init_profile": (_i, [_p, _i, _p]),
            "alifmm_put_field": (_i, [_p, _i, _i, _p]),
            "alifmm_tfm": (_i, [_p, _i, _i, _p, _i, _p, _p, _i, _i, _d, _d, _p, _i, _i, _i, _i, _i, _p]),
            "alifmm_tfm_model": (_i, [_p, _i, _i, _p, _i, _p, _p, _i, _i, _d, _d, _p, _i, _i, _i, _i, _i, _p]),
            "alifmm_tfm_f64": (_i, [_p, _i, _i, _p, _i, _p, _p, _i, _i, _d, _d, _p, _i, _i, _i, _i, _i, _p]),
            "alifmm_tfm_coh": (_i, [_p, _i, _i, _p, _i, _p, _p, _i, _i, _d, _d, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
            "alifmm_tfm_lsq": (_i, [_p, _i, _i, _p, _i, _p, _p, _i, _i, _d, _d, _p, _i, _i, _i, _i, _i, _d, _d, _i, _d,
                                    _p, _p, _p]),
            "alifmm_tfm_lsq_pulse": (_i, [_p, _i, _i, _p, _i, _p, _p, _i, _i, _d, _d, _p, _i, _i, _i, _i, _i, _d, _d, _i,
                                          _d, _i, _i, _p, _i, _p, _p, _p]),
            "alifmm_tfm_sparse": (_i, [_p, _i, _i, _p, _i, _p, _p, _i, _i, _d, _d, _p, _i, _i, _i, _i, _i, _d, _d, _i, _d,
                                       _i, _i, _p, _i, _d, _d, _i, _i, _p, _p, _p]),
            "alifmm_trace_fir": (_i, [_p, _l, _i, _i, _p, _i, _i, _p, _i, _i, _p]),
            "alifmm_trace_spectral": (_i, [_p, _l, _i, _i, _i, _p, _i, _i, _p, _i, _p]),
            "alifmm_trace_pick": (_i, [_p, _l, _i, _i, _i, _p, _i, _i, _i, _p, _i, _p, _p, _i, _d, _i, _p, _p, _p, _p, _p,
                                       _p]),
            "alifmm_ray_sens": (_i, [_p, _i, _i, _p, _p, _p, _p, _p, _p, _l, _p, _p, _p, _p, _p]),
            "alifmm_sens_op_build": (_i, [_p, _i, _i, _p, _p, _p, _i, _p, _p, _p]),
            "alifmm_sens_op_apply": (_i, [_p, _i, _p, _p]),
            "alifmm_sens_op_solve": (_i, [_p, _p, _d, _d, _i, _d, _p, _p]),
            "alifmm_sens_op_release": (_i, [_p]),
            "alifmm_time_between_points": (_i, [_p, _i, _p, _p, _p, _p, _i, _p]),
            "alifmm_local_ops": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i,
                                      _p]),
            "alifmm_cr_math": (_i, [_p, _i, _i, _l, _p, _p, _p]),
            "alifmm_fouds18_band": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p]),
            "alifmm_fouds18_band_lanes": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p]),
            "alifmm_comm_unique_id": (_i, [_p]),
            "alifmm_comm_init_rank": (_i, [_p, _i, _i, _p, _p]),
            "alifmm_comm_init_all": (_i, [_p, _i, _p]),
            "alifmm_comm_destroy": (_i, [_p]),
            "alifmm_comm_last_error": (ctypes.c_char_p, [_p]),
            "alifmm_gather_fields": (_i, [_p, _i, _i, _p, _p, _i, _p]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
        return L


def lib():
    return _load()


def _profiler_attached():
    """True under rocprofv3 (its tool library is configured through ROCPROF* / ROCP_* variables)."""
    return any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ)


def shutdown():
    """Destroy every open context and communicator at interpreter exit (atexit), while the HIP
    runtime is intact: their streams, events, pinned buffers and device memory are released in
    order instead of by the runtime's own static teardown.

    The library stays mapped (its path shows in the process maps to the end, as any loaded
    extension's), except under a profiler: rocprofv3 registers its finalisation after the
    library's HIP module destructor (__hip_module_dtor, registered with __cxa_atexit when the
    library is loaded), so that destructor would run from exit() after the tool has torn down;
    there the library is unloaded here, which runs the destructor now."""
    global _lib, _lib_closed
    live = list(_live)
    for c in [c for c in live if isinstance(c, Comm)] + [c for c in live if not isinstance(c, Comm)]:
        try:
            c.close()
        except Exception:
            pass
    _default.clear()
    if not _profiler_attached():
        return
    with _lock:
        L, _lib, _lib_closed = _lib, None, True
    if L is not None:
        import _ctypes

        _ctypes.dlclose(L._handle)


atexit.register(shutdown)


def device_count():
    n = ctypes.c_int(0)
    lib().alifmm_device_count(ctypes.byref(n))
    return n.value


def _c64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ci64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _ci32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


KEEP_RAYS = -1  # ALIFMM_KEEP_RAYS (include/alifmm.h)


def _ptr(a):
    return None if a is None else a.ctypes.data


class Context:
    """One GPU (HIP device index).  Holds the resident model and travel-time fields."""

    def __init__(self, device=0, cdelta=None, r0=None, batch=None):
        L = lib()
        h = ctypes.c_void_p()
        rc = L.alifmm_ctx_create(int(device), ctypes.byref(h))
        if rc != 0 or not h.value:
            raise AlifmmError("alifmm_ctx_create(device=%d) failed (rc=%d): no usable MI355X/HIP device"
                              % (device, rc))
        self._h = h
        self.device = device
        _live.add(self)
        self._model_key = None
        self.shape = None
        for k, v in (("cdelta", cdelta), ("r0", r0), ("batch", batch)):
            if v is not None:
                self.set_option(k, v)
        # experiments (tools/*.sh): ALIFMM_OPT_<NAME>=value sets alifmm_set_option(name, value) on
        # every context (README "Options"); a bad name or value is reported and ignored, never fatal
        for k, v in os.environ.items():
            if k.startswith("ALIFMM_OPT_"):
                try:
                    self.set_option(k[len("ALIFMM_OPT_"):].lower(), float(v))
                except (ValueError, AlifmmError) as e:
                    import warnings

                    warnings.warn("ignoring %s=%r: %s" % (k, v, e))

    def _chk(self, rc, what):
        if rc != 0:
            msg = lib().alifmm_last_error(self._h)
            raise AlifmmError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ""))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value and _lib is not None:
            _lib.alifmm_ctx_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def model_key(self):
        """Key of the resident model (set_model(key=...)), None when unknown."""
        return self._model_key

    def set_option(self, name, value):
        self._chk(lib().alifmm_set_option(self._h, name.encode(), float(value)), "set_option(%s)" % name)

    def get_option(self, name):
        v = ctypes.c_double(0)
        self._chk(lib().alifmm_get_option(self._h, name.encode(), ctypes.byref(v)), "get_option(%s)" % name)
        return v.value

    def set_model(self, veln, velpn, vel_map, stif_den, group_tab, phase_tab, dnx, dnz=None, gox=0.0, goz=0.0,
                  key=None):
        """Upload the model unless `key` equals the key of the resident model."""
        if key is not None and key == self._model_key:
            return
        veln = _c64(veln)
        nnz, nnx = veln.shape
        velpn = _ci64(velpn)
        vel_map = _c64(vel_map)
        stif = None if stif_den is None else _ci64(stif_den)
        gt = _c64(group_tab)
        pt = _c64(phase_tab if phase_tab is not None else group_tab)
        if velpn.shape != veln.shape or vel_map.shape != veln.shape:
            raise ValueError("veln, velpn and vel_map must have the same shape")
        if stif is not None and stif.shape != (nnz, nnx, 5):
            raise ValueError("stif_den must have shape (nnz, nnx, 5)")
        if gt.ndim != 2 or gt.shape[0] != 361 or pt.shape != gt.shape:
            raise ValueError("velocity tables must have shape (361, ncol)")
        dnz = dnx if dnz is None else dnz
        # forget the resident key first: if the upload fails, the next call must upload again
        self._model_key = None
        self._chk(lib().alifmm_set_model(self._h, nnz, nnx, _ptr(veln), _ptr(velpn), _ptr(vel_map), _ptr(stif),
                                         _ptr(gt), _ptr(pt), gt.shape[1], float(dnx), float(dnz), float(gox),
                                         float(goz)), "set_model")
        self._model_key = key
        self.shape = (nnz, nnx)

    def field_shape(self, subgrid):
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(lib().alifmm_field_shape(self._h, int(subgrid), ctypes.byref(a), ctypes.byref(b)), "field_shape")
        return a.value, b.value

    def travel(self, scx, scz, subgrid=1, first_slot=0, copy_out=True):
        """Travel-time fields for sources (scx, scz) [m]; resident in slots first_slot.. ."""
        scx = _c64(np.atleast_1d(scx))
        scz = _c64(np.atleast_1d(scz))
        fz, fx = self.field_shape(subgrid)
        out = np.empty((len(scx), fz, fx)) if copy_out else None
        self._chk(lib().alifmm_travel(self._h, int(subgrid), len(scx), _ptr(scx), _ptr(scz), int(first_slot),
                                      _ptr(out)), "travel")
        return out

    def travel_into(self, scx, scz, dest, rows, subgrid=1, first_slot=0):
        """travel() with field i written to dest[rows[i]] of a caller-visible C-contiguous float64
        (n, fnz, fnx) stack (alifmm_travel_into: at subgrid 1 the fields stream out of the band
        kernel tile by tile while it runs).  The fields also stay resident in slots first_slot.. ."""
        scx = _c64(np.atleast_1d(scx))
        scz = _c64(np.atleast_1d(scz))
        if not (isinstance(dest, np.ndarray) and dest.dtype == np.float64 and dest.flags.c_contiguous
                and dest.ndim == 3):
            raise ValueError("dest must be a C-contiguous float64 (n, fnz, fnx) array")
        if dest.shape[1:] != self.field_shape(subgrid):
            raise ValueError("dest fields %s, travel fields %s" % (dest.shape[1:], self.field_shape(subgrid)))
        rows = [int(r) for r in rows]
        if len(rows) != len(scx):
            raise ValueError("one dest row per source")
        if rows and (min(rows) < 0 or max(rows) >= dest.shape[0]):
            raise IndexError("travel_into: row outside dest")
        base, step = dest.ctypes.data, dest[0].nbytes if dest.shape[0] else 0
        ptrs = (ctypes.c_void_p * max(1, len(rows)))(*[base + r * step for r in rows])
        self._chk(lib().alifmm_travel_into(self._h, int(subgrid), len(scx), _ptr(scx), _ptr(scz), int(first_slot),
                                           ptrs), "travel_into")

    def travel_seeded(self, seed_iz, seed_ix, times=None, from_slots=None, first_slot=0, copy_out=True):
        """Subgrid-1 travel-time fields from seed nodes (seed_iz[k], seed_ix[k]) with given times
        (alifmm_travel_seeded): reflected legs and fronts that are no points.

        times: (nseed,) for one field or (nfield, nseed) host times; or from_slots: resident
        subgrid-1 slots, field i taking its seed times from field from_slots[i] at the seed nodes, on
        the device.  Exactly one of the two.  The seeds keep their times; the fields land in slots
        first_slot.. and stay resident.  Seeds plus their non-seed 4-neighbours must fit 11 881
        entries.  Returns (nfield, nnz, nnx), or None with copy_out=False."""
        iz, ix = _ci32(np.atleast_1d(seed_iz)), _ci32(np.atleast_1d(seed_ix))
        if iz.ndim != 1 or iz.shape != ix.shape:
            raise ValueError("seed_iz and seed_ix must be one-dimensional and of one length")
        t = fs = None
        nfield = 1  # neither source of times: the library refuses the call
        if times is not None:
            t = np.atleast_2d(_c64(times))
            if t.ndim != 2 or t.shape[1] != len(iz):
                raise ValueError("times must have shape (nseed,) or (nfield, nseed)")
            nfield = t.shape[0]
        if from_slots is not None:
            fs = _ci32(np.atleast_1d(from_slots))
            nfield = len(fs) if times is None else nfield
        out = np.empty((nfield,) + tuple(self.shape)) if copy_out and self.shape is not None and nfield else None
        self._chk(lib().alifmm_travel_seeded(self._h, nfield, len(iz), _ptr(iz), _ptr(ix), _ptr(t), _ptr(fs),
                                             int(first_slot), _ptr(out)), "travel_seeded")
        return out

    def get_field(self, slot, subgrid):
        fz, fx = self.field_shape(subgrid)
        out = np.empty((fz, fx))
        self._chk(lib().alifmm_get_field(self._h, int(slot), _ptr(out)), "get_field")
        return out

    def put_field(self, slot, subgrid, data):
        data = _c64(data)
        if data.shape != self.field_shape(subgrid):
            raise ValueError("field shape %s does not match subgrid %d" % (data.shape, subgrid))
        self._chk(lib().alifmm_put_field(self._h, int(slot), int(subgrid), _ptr(data)), "put_field")

    def _tfm_args(self, what, tx_slots, rx_slots, fmc, weights, window, step, subgrid, f64):
        """The arguments tfm() and tfm_lsq() share: (tx, rx, data, complex?, weights, window)."""
        tx, rx = _ci32(np.atleast_1d(tx_slots)), _ci32(np.atleast_1d(rx_slots))
        fmc = np.asarray(fmc)
        if fmc.ndim != 3 or fmc.shape[:2] != (len(tx), len(rx)):
            raise ValueError("fmc must have shape (ntx, nrx, nt) = (%d, %d, nt), not %s"
                             % (len(tx), len(rx), fmc.shape))
        cplx = np.iscomplexobj(fmc)
        if f64:
            data = np.ascontiguousarray(fmc, dtype=np.complex128 if cplx else np.float64)
        else:
            data = np.ascontiguousarray(fmc, dtype=np.complex64 if cplx else np.float32)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != fmc.shape[:2]:
                raise ValueError("weights must have shape (ntx, nrx)")
        if window is None:
            if step < 1:
                raise AlifmmError("%s: step %d" % (what, step))
            fz, fx = self.field_shape(subgrid)
            window = (0, 0, (fz - 1) // step + 1, (fx - 1) // step + 1)
        return tx, rx, data, cplx, w, tuple(int(v) for v in window)

    def tfm(self, tx_slots, rx_slots, fmc, fs, t0=0.0, weights=None, window=None, step=1, subgrid=1, precision="f32"):
        """Total-focusing-method image of full-matrix-capture data over resident fields
        (alifmm_tfm): I(p) = sum_ab w_ab s_ab(T_a(p) + T_b(p)), linear interpolation in time, all
        in float64; the fields stay on the device and one image comes back.

        tx_slots, rx_slots: resident slots (of `subgrid`, one shape) of the transmitters' and
        receivers' fields.  fmc: (ntx, nrx, nt) real RF or complex analytic data (any float or
        complex dtype; sent as float32 / interleaved float32), sample k taken at t0 + k / fs.
        weights: (ntx, nrx) or None.  window = (iz0, ix0, niz, nix) in pixels of `step` fine-grid
        nodes from node (iz0, ix0); None: the whole field at that step.
        precision: "f32" (the default) sends the data as float32; "f64" sends them as float64
        (alifmm_tfm_f64: the same sum in the same order, the samples read as they are; on data that
        float32 represents exactly, the same bits).
        Returns float64 (niz, nix), or complex128 for complex data."""
        if precision not in ("f32", "f64"):
            raise ValueError("tfm: precision %r is neither 'f32' nor 'f64'" % (precision,))
        step = int(step)
        f64 = precision == "f64"
        tx, rx, data, cplx, w, window = self._tfm_args("tfm", tx_slots, rx_slots, fmc, weights, window, step, subgrid, f64)
        iz0, ix0, niz, nix = window
        nc = 2 if cplx else 1
        img = np.empty((max(niz, 0), max(nix, 0), nc))
        call = lib().alifmm_tfm_f64 if f64 else lib().alifmm_tfm
        self._chk(call(self._h, int(subgrid), len(tx), _ptr(tx), len(rx), _ptr(rx), _ptr(data), data.shape[2], nc,
                       float(t0), float(fs), _ptr(w), iz0, ix0, niz, nix, step, _ptr(img)), "tfm")
        return img.view(np.complex128)[..., 0] if cplx else img[..., 0]

    COHERENCE_KINDS = {"cf": 1, "scf": 2, "pcf": 3}

    def tfm_coh(self, tx_slots, rx_slots, fmc, fs, kind="cf", t0=0.0, weights=None, window=None, step=1, subgrid=1,
                sums=False):
        """tfm() together with a per-pixel coherence factor in [0, 1] from a second sum over the
        same terms, made in the same pass over the resident fields (alifmm_tfm_coh).

        kind: "cf" the coherence factor |sum t|² / (n sum |t|²); "scf" the sign coherence factor
        1 - sqrt(1 - (sum sign Re t / n)²); "pcf" the phase coherence factor
        1 - sqrt(1 - |sum t / |t||² / n²), complex data only; n counts the terms in range.
        tx_slots, rx_slots, fmc, fs, t0, weights, window, step, subgrid: as in tfm(), the data sent
        as float32.
        Returns (image, factor), or (image, factor, sums) with sums=True: image as tfm() returns it,
        to the bit; factor float64 (niz, nix); sums float64 (niz, nix, 3), the raw sums (n, q, 0),
        (n, b, 0) or (n, ph_re, ph_im) of the kind.  The weighted image is image * factor ** p."""
        if kind not in self.COHERENCE_KINDS:
            raise ValueError("tfm_coh: kind %r is none of 'cf', 'scf', 'pcf'" % (kind,))
        step = int(step)
        tx, rx, data, cplx, w, window = self._tfm_args("tfm_coh", tx_slots, rx_slots, fmc, weights, window, step, subgrid,
                                                       False)
        iz0, ix0, niz, nix = window
        nc = 2 if cplx else 1
        img = np.empty((max(niz, 0), max(nix, 0), nc))
        fac = np.empty(img.shape[:2])
        raw = np.empty(img.shape[:2] + (3,)) if sums else None
        self._chk(lib().alifmm_tfm_coh(self._h, int(subgrid), len(tx), _ptr(tx), len(rx), _ptr(rx), _ptr(data),
                                       data.shape[2], nc, float(t0), float(fs), _ptr(w), iz0, ix0, niz, nix, step,
                                       self.COHERENCE_KINDS[kind], _ptr(img), _ptr(fac), _ptr(raw)), "tfm_coh")
        image = img.view(np.complex128)[..., 0] if cplx else img[..., 0]
        return (image, fac, raw) if sums else (image, fac)

    @staticmethod
    def _pulse_args(what, pulse, cplx_data):
        """A 1-D real or complex pulse -> its taps, float64 (ntap, tap_comp)."""
        pulse = np.asarray(pulse)
        if pulse.ndim != 1:
            raise ValueError("%s: pulse must be a 1-D array, not %s" % (what, pulse.shape))
        if np.iscomplexobj(pulse):
            if not cplx_data:
                raise ValueError("%s: a complex pulse needs complex data" % what)
            return np.ascontiguousarray(pulse, dtype=np.complex128).view(np.float64).reshape(-1, 2)
        return np.ascontiguousarray(pulse, dtype=np.float64).reshape(-1, 1)

    def trace_fir(self, data, pulse, origin=0, transpose=False):
        """Every trace of data convolved with one pulse on the device (alifmm_trace_fir), or, with
        transpose=True, correlated with it: the exact transpose of the same linear map.
        out[..., t] = sum_j pulse[j] data[..., t - j + origin], j ascending, samples outside the
        trace adding nothing; transposed, out[..., t] = sum_j conj(pulse[j]) data[..., t + j - origin].
        All in float64 in a fixed order: the result is reproducible to the bit and a trace does not
        depend on the others.

        data: (..., nt) real or complex, sent as float64.  pulse: 1-D real or complex, at most 1024
        finite taps; a complex pulse needs complex data.  origin: the tap index of the pulse's time
        zero (0: causal, the convention of ALI_FMM.simulate_fmc).
        Returns float64, or complex128 for complex data, of data's shape."""
        data = np.asarray(data)
        if data.ndim < 1:
            raise ValueError("trace_fir: data must have shape (..., nt)")
        cplx = np.iscomplexobj(data)
        taps = self._pulse_args("trace_fir", pulse, cplx)
        x = np.ascontiguousarray(data, dtype=np.complex128 if cplx else np.float64)
        nc = 2 if cplx else 1
        nt = x.shape[-1]
        out = np.empty(x.shape + (nc,))
        self._chk(lib().alifmm_trace_fir(self._h, x.size // nt if nt else 0, nt, nc, _ptr(x), taps.shape[0], taps.shape[1],
                                         _ptr(taps), int(origin), int(bool(transpose)), _ptr(out)), "trace_fir")
        return out.view(np.complex128)[..., 0] if cplx else out[..., 0]

    def trace_spectral(self, data, response=None, analytic=False, nfft=None):
        """Every trace of data filtered in the frequency domain on the device
        (alifmm_trace_spectral): out = IDFT(G · DFT(data)) over nfft points, G the analytic mask
        (analytic=True: scipy.signal.hilbert(data, N=nfft)[..., :nt]), the response, or both.  A
        radix-2 transform in float64 with a written-out operation order (include/alifmm.h): the
        result is reproducible to the bit and a trace does not depend on the others.

        data: (..., nt) real or complex, nt <= 8192; float32 and complex64 are sent as float32, any
        other dtype as float64.  nfft: a power of two in [nt, 8192]; None: the smallest one >= nt
        (the trace is zero-padded to it and the result cut to nt).  response: None, or (nfft,) real
        or complex, H_k at bin k in numpy.fft's order (bandpass_response() makes one), all finite.
        Returns complex64 for float32 / complex64 data, else complex128, of data's shape."""
        x, cplx, f32 = self._trace_args("trace_spectral", data)
        nt = x.shape[-1]
        h, hc = self._response_args("trace_spectral", response, nt, nfft)
        out = np.empty(x.shape, dtype=np.complex64 if f32 else np.complex128)
        self._chk(lib().alifmm_trace_spectral(self._h, x.size // nt if nt else 0, nt, 2 if cplx else 1, int(f32), _ptr(x),
                                              int(nfft) if nfft else 0, hc, _ptr(h), int(bool(analytic)), _ptr(out)),
                  "trace_spectral")
        return out

    @staticmethod
    def _trace_args(what, data):
        """Traces as trace_spectral and trace_pick send them: (contiguous array, complex, float32)."""
        data = np.asarray(data)
        if data.ndim < 1:
            raise ValueError("%s: data must have shape (..., nt)" % what)
        cplx = np.iscomplexobj(data)
        f32 = data.dtype in (np.float32, np.complex64)
        x = np.ascontiguousarray(data, dtype=(np.complex64 if cplx else np.float32) if f32
                                 else (np.complex128 if cplx else np.float64))
        return x, cplx, f32

    @staticmethod
    def _response_args(what, response, nt, nfft):
        """A frequency response as the same two send it: (float64 or complex128 array or None, its
        components 0, 1 or 2)."""
        if response is None:
            return None, 0
        n = int(nfft) if nfft else 1 << max(nt - 1, 0).bit_length()
        response = np.asarray(response)
        if response.shape != (n,):
            raise ValueError("%s: response must have shape (nfft,) = (%d,), not %s" % (what, n, response.shape))
        hc = 2 if np.iscomplexobj(response) else 1
        return np.ascontiguousarray(response, dtype=np.complex128 if hc == 2 else np.float64), hc

    def trace_pick(self, data, gate_lo, gate_hi, mode="peak", frac=0.5, guard=0, response=None, analytic=False, nfft=None):
        """Time-of-flight picks on the device (alifmm_trace_pick): per trace the largest |sample|
        inside the gate [gate_lo, gate_hi) (mode="peak"), or the first sample of the gate that
        reaches frac of it (mode="onset", 0 < frac <= 1), refined to a fraction of a sample, and the
        largest |sample| more than guard samples away from the peak.  With a response or
        analytic=True the traces first pass trace_spectral()'s filter (its arguments and limits)
        and are picked where it left them on the device: only the picks come back, and they are,
        to the bit, those of trace_pick(trace_spectral(data, ...), ...).  The rules are written out
        operation by operation in include/alifmm.h: the picks are reproducible to the bit and a
        trace does not depend on the others.

        data: (..., nt) real or complex; float32 and complex64 are sent as float32, any other dtype
        as float64.  gate_lo, gate_hi: integers shaped like data's leading dimensions (or
        broadcastable to them), 0 <= lo, hi <= nt; lo >= hi: the trace is not asked for.
        Returns (pos, amp, idx, amp2, idx2, flags), each shaped like the leading dimensions: the
        pick in samples (NaN: none), the peak's amplitude and sample, the runner-up's amplitude and
        sample (-1: none), and flags (1 no gate, 2 nothing to pick, 4 unrefined, 8 at the gate's
        edge, 16 a non-finite sample in the gate)."""
        x, cplx, f32 = self._trace_args("trace_pick", data)
        nt = x.shape[-1]
        lead = x.shape[:-1]
        m = {"peak": 0, "onset": 1}.get(mode)
        if m is None:
            raise ValueError("trace_pick: mode must be 'peak' or 'onset'")
        try:
            lo = np.ascontiguousarray(np.broadcast_to(np.asarray(gate_lo), lead), dtype=np.int32)
            hi = np.ascontiguousarray(np.broadcast_to(np.asarray(gate_hi), lead), dtype=np.int32)
        except ValueError:
            raise ValueError("trace_pick: the gates must have data's leading shape %s" % (lead,)) from None
        filt = response is not None or bool(analytic)
        h, hc = self._response_args("trace_pick", response, nt, nfft) if filt else (None, 0)
        if not filt and nfft:
            raise ValueError("trace_pick: nfft needs a response or analytic=True")
        pos, amp, amp2 = (np.empty(lead) for _ in range(3))
        idx, idx2, flags = (np.empty(lead, dtype=np.int32) for _ in range(3))
        self._chk(lib().alifmm_trace_pick(self._h, x.size // nt if nt else 0, nt, 2 if cplx else 1, int(f32), _ptr(x),
                                          int(filt), int(nfft) if nfft else 0, hc, _ptr(h), int(bool(analytic)), _ptr(lo),
                                          _ptr(hi), m, float(frac), int(guard), _ptr(pos), _ptr(amp), _ptr(idx), _ptr(amp2),
                                          _ptr(idx2), _ptr(flags)), "trace_pick")
        return pos, amp, idx, amp2, idx2, flags

    def tfm_lsq(self, tx_slots, rx_slots, fmc, fs, t0=0.0, weights=None, window=None, step=1, subgrid=1, damp=0.0,
                smooth=0.0, max_iter=50, tol=1e-6, resid=False, pulse=None, pulse_origin=0):
        """Least-squares image of full-matrix-capture data over resident fields (alifmm_tfm_lsq):
        CGLS from x = 0 on min |A x - fmc|² + damp² |x|² + smooth² |D x|², A being tfm_model() on
        the dense window, Aᵀ tfm(precision="f64") and D the first difference between 4-neighbour
        pixels.  The data, every vector and every scalar of the iteration stay on the device; one
        image comes back.  A sums with atomics, so two solves agree to rounding, not to the bit,
        and their iteration counts may differ by one.

        tx_slots, rx_slots, fs, t0, weights, window, step, subgrid: as in tfm().  fmc: (ntx, nrx,
        nt) real or complex, every value finite, sent as float64.  damp is absolute (|A|_2 is of the
        order sqrt(ntx nrx)).
        pulse: None, or the transducer's pulse, 1-D real or complex (complex: complex data), at
        most 1024 finite taps, with pulse_origin the tap index of its time zero.  The operator is
        then P A (alifmm_tfm_lsq_pulse), P being trace_fir(., pulse, pulse_origin) on every trace:
        the model of measured data, which are the spike trains of tfm_model() convolved with the
        pulse.  grad0 = |Aᵀ Pᵀ fmc|, and the residual is fmc - P A x.
        Returns (image, info), or (image, info, resid) with resid=True (the recurred residual, the
        shape of fmc): image float64 (niz, nix) or complex128 for complex data; info =
        dict(iterations, grad0 = |Aᵀ fmc|, grad, rhs_norm, res_norm, reason ("tol", "max_iter" or
        "breakdown"))."""
        step = int(step)
        tx, rx, data, cplx, w, window = self._tfm_args("tfm_lsq", tx_slots, rx_slots, fmc, weights, window, step, subgrid,
                                                       True)
        iz0, ix0, niz, nix = window
        nc = 2 if cplx else 1
        img = np.zeros((max(niz, 0), max(nix, 0), nc))
        res = np.zeros(data.shape + (nc,)) if resid else None
        info = np.zeros(8)
        head = (self._h, int(subgrid), len(tx), _ptr(tx), len(rx), _ptr(rx), _ptr(data), data.shape[2], nc, float(t0),
                float(fs), _ptr(w), iz0, ix0, niz, nix, step, float(damp), float(smooth), int(max_iter), float(tol))
        if pulse is None:
            self._chk(lib().alifmm_tfm_lsq(*head, _ptr(img), _ptr(res), _ptr(info)), "tfm_lsq")
        else:
            taps = self._pulse_args("tfm_lsq", pulse, cplx)
            self._chk(lib().alifmm_tfm_lsq_pulse(*head, taps.shape[0], taps.shape[1], _ptr(taps), int(pulse_origin),
                                                 _ptr(img), _ptr(res), _ptr(info)), "tfm_lsq")
        out = {"iterations": int(info[0]), "grad0": info[1], "grad": info[2], "rhs_norm": info[3], "res_norm": info[4],
               "reason": self.SOLVE_REASONS[int(info[5])]}
        image = img.view(np.complex128)[..., 0] if cplx else img[..., 0]
        if not resid:
            return image, out
        return image, out, (res.view(np.complex128)[..., 0] if cplx else res[..., 0])

    def tfm_sparse(self, tx_slots, rx_slots, fmc, fs, t0=0.0, weights=None, window=None, step=1, subgrid=1, damp=0.0,
                   smooth=0.0, max_iter=500, tol=1e-6, resid=False, pulse=None, pulse_origin=0, lam=None, lam_rel=None,
                   lipschitz=0.0, power_iters=20, restart=True):
        """Sparsity-regularised image of full-matrix-capture data over resident fields
        (alifmm_tfm_sparse): the minimiser of ½ |P A x - fmc|² + ½ damp² |x|² + ½ smooth² |D x|² +
        lam Σ_pixels |x_p| by FISTA with backtracking and gradient restart from x = 0.  A, P, D, damp
        and smooth are tfm_lsq()'s; |x_p| is the modulus of a pixel (a complex pixel is one group,
        its phase is not penalised).  The data and every vector of the iteration stay on the
        device; one image comes back.  A sums with atomics, so two solves agree to rounding only.

        tx_slots ... subgrid, damp, smooth, pulse, pulse_origin: as in tfm_lsq().  lam: the weight
        of the ℓ1 term in the units of the gradient Aᵀ Pᵀ fmc; lam_rel: the same in units of
        lam_max = max_p |(Aᵀ Pᵀ fmc)_p|, the smallest lam whose minimiser is 0 (the library takes
        lam_max from its own first gradient; a negative lam means the same, as at the C level).
        Exactly one of the two.  lipschitz: an estimate of
        |BᵀB + R|₂, or 0 for power_iters rounds of the power method; it is doubled whenever a step
        fails its descent test.  restart: gradient restart of the momentum.  The stop rule is
        L |x⁺ - y| <= tol grad0.
        Returns (image, info), or (image, info, resid) with resid=True (fmc - P A image, computed):
        info = dict(iterations, grad0 = |Aᵀ Pᵀ fmc|, grad (the last L |x⁺ - y|), rhs_norm, res_norm,
        reason ("tol", "max_iter" or "breakdown"), lam_max, lam, lipschitz (the final L),
        backtracks, restarts, nnz (non-zero pixels))."""
        if (lam is None) == (lam_rel is None):
            raise ValueError("tfm_sparse: give exactly one of lam and lam_rel")
        if lam_rel is not None and not float(lam_rel) >= 0:
            raise ValueError("tfm_sparse: lam_rel %r is negative or not a number" % (lam_rel,))
        step = int(step)
        tx, rx, data, cplx, w, window = self._tfm_args("tfm_sparse", tx_slots, rx_slots, fmc, weights, window, step,
                                                       subgrid, True)
        iz0, ix0, niz, nix = window
        nc = 2 if cplx else 1
        img = np.zeros((max(niz, 0), max(nix, 0), nc))
        res = np.zeros(data.shape + (nc,)) if resid else None
        info = np.zeros(12)
        taps = None if pulse is None else self._pulse_args("tfm_sparse", pulse, cplx)
        # (a relative lam travels as its negative; -0.0 is the absolute 0, the same problem)
        self._chk(lib().alifmm_tfm_sparse(
            self._h, int(subgrid), len(tx), _ptr(tx), len(rx), _ptr(rx), _ptr(data), data.shape[2], nc, float(t0),
            float(fs), _ptr(w), iz0, ix0, niz, nix, step, float(damp), float(smooth), int(max_iter), float(tol),
            0 if taps is None else taps.shape[0], 1 if taps is None else taps.shape[1], _ptr(taps), int(pulse_origin),
            float(lam) if lam is not None else -float(lam_rel), float(lipschitz), int(power_iters), int(bool(restart)),
            _ptr(img), _ptr(res), _ptr(info)), "tfm_sparse")
        out = {"iterations": int(info[0]), "grad0": info[1], "grad": info[2], "rhs_norm": info[3], "res_norm": info[4],
               "reason": self.SOLVE_REASONS[int(info[5])], "lam_max": info[6], "lam": info[7], "lipschitz": info[8],
               "backtracks": int(info[9]), "restarts": int(info[10]), "nnz": int(info[11])}
        image = img.view(np.complex128)[..., 0] if cplx else img[..., 0]
        if not resid:
            return image, out
        return image, out, (res.view(np.complex128)[..., 0] if cplx else res[..., 0])

    def tfm_model(self, tx_slots, rx_slots, refl, fs, nt, t0=0.0, weights=None, window=None, step=1, subgrid=1):
        """Full-matrix-capture data a reflectivity map predicts under the delay laws of resident
        fields (alifmm_tfm_model), the exact transpose of tfm(): pixel p adds w_ab refl(p), split
        linearly over the two samples around T_a(p) + T_b(p), to the trace of every pair (a, b); all
        in float64.  The fields stay on the device and the data come back.  The order of the sums
        is not fixed: two calls agree to rounding, not to the bit.

        tx_slots, rx_slots, fs, t0, weights, window, step, subgrid: as in tfm().  refl: (niz, nix)
        real or complex on the pixel window, every value finite; zero pixels cost nothing.  nt:
        samples per trace.  Returns float64 (ntx, nrx, nt), or complex128 when refl is complex."""
        tx, rx = _ci32(np.atleast_1d(tx_slots)), _ci32(np.atleast_1d(rx_slots))
        refl = np.asarray(refl)
        cplx = np.iscomplexobj(refl)
        step = int(step)
        if window is None:
            if step < 1:
                raise AlifmmError("tfm_model: step %d" % step)
            fz, fx = self.field_shape(subgrid)
            window = (0, 0, (fz - 1) // step + 1, (fx - 1) // step + 1)
        iz0, ix0, niz, nix = (int(v) for v in window)
        if refl.ndim != 2 or refl.shape != (max(niz, 0), max(nix, 0)):
            raise ValueError("refl must have the window's shape (%d, %d), not %s" % (niz, nix, refl.shape))
        x = np.ascontiguousarray(refl, dtype=np.complex128 if cplx else np.float64)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != (len(tx), len(rx)):
                raise ValueError("weights must have shape (ntx, nrx)")
        nc = 2 if cplx else 1
        nt = int(nt)
        out = np.empty((len(tx), len(rx), max(nt, 0), nc))
        self._chk(lib().alifmm_tfm_model(self._h, int(subgrid), len(tx), _ptr(tx), len(rx), _ptr(rx), _ptr(x), nc, nt,
                                         float(t0), float(fs), _ptr(w), iz0, ix0, niz, nix, step, _ptr(out)),
                  "tfm_model")
        return out.view(np.complex128)[..., 0] if cplx else out[..., 0]

    def copy_fields(self, first_slot, n, subgrid, out=None, dst_kind=0):
        """Resident fields of slots first_slot .. first_slot+n-1 as one (n, fnz, fnx) host array
        (alifmm_copy_fields: pageable destinations go through the pinned staging ring).
        Returns (array, GB/s)."""
        fz, fx = self.field_shape(subgrid)
        if out is None:
            out = np.empty((n, fz, fx))
        g = ctypes.c_double(0)
        self._chk(lib().alifmm_copy_fields(self._h, int(first_slot), int(n), _ptr(out), int(dst_kind), ctypes.byref(g)),
                  "copy_fields")
        return out, g.value

    def copy_fields_into(self, first_slot, dest, rows, subgrid, dst_kind=0):
        """Resident slots first_slot, first_slot+1, ... straight into dest[rows[0]], dest[rows[1]], ...
        of a caller-visible C-contiguous float64 (n, fnz, fnx) stack: one copy per field, no
        intermediate array (runs of consecutive rows go in one alifmm_copy_fields call).
        dst_kind 0: through the pinned staging ring; 3: DMA straight into dest (registered for the
        copy).  Returns the bytes copied."""
        if not (isinstance(dest, np.ndarray) and dest.dtype == np.float64 and dest.flags.c_contiguous
                and dest.ndim == 3):
            raise ValueError("dest must be a C-contiguous float64 (n, fnz, fnx) array")
        if dest.shape[1:] != self.field_shape(subgrid):
            raise ValueError("dest fields %s, resident fields %s" % (dest.shape[1:], self.field_shape(subgrid)))
        rows = [int(r) for r in rows]
        if rows and (min(rows) < 0 or max(rows) >= dest.shape[0]):
            raise IndexError("copy_fields_into: row outside dest")
        g = ctypes.c_double(0)
        k = 0
        while k < len(rows):
            e = k + 1
            while e < len(rows) and rows[e] == rows[e - 1] + 1:
                e += 1
            self._chk(lib().alifmm_copy_fields(self._h, int(first_slot + k), e - k, dest[rows[k]].ctypes.data,
                                               int(dst_kind), ctypes.byref(g)), "copy_fields")
            k = e
        return len(rows) * dest[0].nbytes

    def copy_fields_to_device(self, first_slot, n, dev_ptr):
        """Copy resident fields into device memory of this GPU at dev_ptr (e.g. a torch tensor's
        data_ptr(), for an RCCL gather).  Returns GB/s."""
        g = ctypes.c_double(0)
        self._chk(lib().alifmm_copy_fields(self._h, int(first_slot), int(n), ctypes.c_void_p(int(dev_ptr)), 2,
                                           ctypes.byref(g)), "copy_fields")
        return g.value

    def release_fields(self):
        self._chk(lib().alifmm_release_fields(self._h), "release_fields")

    def find_rays(self, slots, src_xy, rec_xy, with_points=True, packed=False, check=True):
        """Rays through resident receiver fields.

        Returns (times, lens, flags, rays): rays is a list of (x, z) arrays per ray, or with
        packed=True one (sum(lens), 2) array of all points in ray order (ray k starts at row
        sum(lens[:k])) — no per-ray copies, and the host buffer is sized exactly (the points wait
        in the context between alifmm_find_rays and alifmm_take_rays).  check: raise
        (check_ray_flags) for a ray cut short at the point capacity or on an empty search plane."""
        slots = _ci32(slots)
        n = len(slots)
        src_xy = _c64(src_xy).reshape(n, 2)
        rec_xy = _c64(rec_xy).reshape(n, 2)
        times = np.zeros(n)
        lens = np.zeros(n, dtype=np.int32)
        flags = np.zeros(n, dtype=np.int32)
        keep = with_points and n > 0
        self._chk(lib().alifmm_find_rays(self._h, n, _ptr(slots), _ptr(src_xy), _ptr(rec_xy), _ptr(times),
                                         _ptr(lens), _ptr(flags), None, KEEP_RAYS if keep else 0), "find_rays")
        if check:
            check_ray_flags(flags)
        if not with_points:
            return times, lens, flags, None
        npts = int(lens.sum(dtype=np.int64))
        pts = np.empty((npts, 2))
        if keep:
            got = ctypes.c_int64(0)
            self._chk(lib().alifmm_take_rays(self._h, _ptr(pts), npts, ctypes.byref(got)), "take_rays")
            if got.value != npts:
                raise AlifmmError("take_rays: %d points kept, %d expected" % (got.value, npts))
        if packed:
            return times, lens, flags, pts
        rays = []
        off = 0
        for k in range(n):
            p = pts[off:off + lens[k]]
            rays.append((p[:, 0].copy(), p[:, 1].copy()))
            off += lens[k]
        return times, lens, flags, rays

    @staticmethod
    def _skip_request(slots_a, slots_b, w_iz, w_ix):
        sa, sb = _ci32(np.atleast_1d(slots_a)), _ci32(np.atleast_1d(slots_b))
        iz, ix = _ci32(np.atleast_1d(w_iz)), _ci32(np.atleast_1d(w_ix))
        if sa.ndim != 1 or sa.shape != sb.shape:
            raise ValueError("slots_a and slots_b must be one-dimensional and of one length")
        if iz.ndim != 1 or iz.shape != ix.shape:
            raise ValueError("w_iz and w_ix must be one-dimensional and of one length")
        return sa, sb, iz, ix

    def skip_pick(self, slots_a, slots_b, w_iz, w_ix):
        """The first back-wall echo of element pairs (alifmm_skip_pick): for pair k the reflector node
        q with the least finite T_a + T_b of the resident fields slots_a[k], slots_b[k] at the nodes
        (w_iz[q], w_ix[q]) of their fine grid; of equal sums the lowest q.
        Returns (pick_time float64, hit int32): hit -1 and pick_time +inf where no sum is finite."""
        sa, sb, iz, ix = self._skip_request(slots_a, slots_b, w_iz, w_ix)
        n = len(sa)
        pick, hit = np.full(n, np.inf), np.full(n, -1, dtype=np.int32)
        self._chk(lib().alifmm_skip_pick(self._h, n, _ptr(sa), _ptr(sb), len(iz), _ptr(iz), _ptr(ix), _ptr(pick),
                                         _ptr(hit)), "skip_pick")
        return pick, hit

    def skip_rays(self, slots_a, slots_b, a_xy, b_xy, w_iz, w_ix, with_points=True, check=True):
        """Echo paths a -> reflector -> b (alifmm_skip_rays): the pick of skip_pick, then the two legs
        hit -> a (through field slots_a[k]) and hit -> b (through slots_b[k]) joined into one ray
        a .. hit .. b.  a_xy, b_xy: the elements' (x, z) on the fine grid.

        Returns (pick_time, hit, times, lens, flags, points): times = t_A + t_B of the legs; flags
        the legs' bits or'ed, RAY_NO_HIT (8) for a pair without a hit (no points); points the packed
        (sum(lens), 2) array in pair order, or None with with_points=False.  The points wait in the
        context as after find_rays, so ray_sens / sens_op_build with ray_xy=None called before the
        points are taken (with_points="keep": they stay kept, points is None) read them in place.
        check: raise (check_ray_flags) for a leg cut short."""
        sa, sb, iz, ix = self._skip_request(slots_a, slots_b, w_iz, w_ix)
        n = len(sa)
        a_xy, b_xy = _c64(a_xy).reshape(n, 2), _c64(b_xy).reshape(n, 2)
        pick, hit = np.full(n, np.inf), np.full(n, -1, dtype=np.int32)
        times, lens, flags = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        keep = bool(with_points) and n > 0
        self._chk(lib().alifmm_skip_rays(self._h, n, _ptr(sa), _ptr(sb), _ptr(a_xy), _ptr(b_xy), len(iz), _ptr(iz),
                                         _ptr(ix), _ptr(pick), _ptr(hit), _ptr(times), _ptr(lens), _ptr(flags), None,
                                         KEEP_RAYS if keep else 0), "skip_rays")
        if check:
            check_ray_flags(flags)
        if not with_points or with_points == "keep":
            return pick, hit, times, lens, flags, None
        npts = int(lens.sum(dtype=np.int64))
        pts = np.empty((npts, 2))
        if keep:
            got = ctypes.c_int64(0)
            self._chk(lib().alifmm_take_rays(self._h, _ptr(pts), npts, ctypes.byref(got)), "take_rays")
            if got.value != npts:
                raise AlifmmError("take_rays: %d points kept, %d expected" % (got.value, npts))
        return pick, hit, times, lens, flags, pts

    def ray_sens(self, ray_len, ray_xy=None, subgrid=1, flags=None, weights=None, maps=True, rows=False):
        """Travel-time sensitivities along rays (alifmm_ray_sens): per piece of every ray the coarse
        cell, the length [m], the time [s] and the time's derivative in the cell's orientation
        [s / degree].

        ray_len: points per ray; ray_xy: their packed (sum(ray_len), 2) points on the fine grid of
        `subgrid`, or None for the points the last find_rays kept on the device
        (alifmm_find_rays(..., NULL, ALIFMM_KEEP_RAYS)); flags: find_rays' flags (rays cut short are
        skipped); weights: per-ray weights of the maps.
        Returns (maps, csr, status): maps (3, nnz, nnx) = sums of w len, w time, w dth per cell, or
        None; csr = (row_ptr, col, len, time, dth) with rows=True, or None; status: 1 for an invalid
        ray (a non-finite point, a cell outside the grid, an unending segment), which has no entries."""
        lens = _ci32(np.atleast_1d(ray_len))
        n = len(lens)
        xy = None
        if ray_xy is not None:
            xy = _c64(ray_xy).reshape(-1, 2)
            if len(xy) != int(np.maximum(lens, 0).sum(dtype=np.int64)):
                raise ValueError("ray_xy holds %d points, ray_len adds up to %d"
                                 % (len(xy), int(np.maximum(lens, 0).sum(dtype=np.int64))))
        fl = None if flags is None else _ci32(np.atleast_1d(flags))
        w = None if weights is None else _c64(np.atleast_1d(weights))
        if (fl is not None and len(fl) != n) or (w is not None and len(w) != n):
            raise ValueError("flags and weights must have one value per ray")
        status = np.zeros(n, dtype=np.int32)
        L = lib()

        def call(m, rp, cap, arrays):
            self._chk(L.alifmm_ray_sens(self._h, int(subgrid), n, _ptr(lens), _ptr(fl), _ptr(xy), _ptr(w), _ptr(m),
                                        _ptr(rp), cap, *[_ptr(a) for a in arrays], _ptr(status)), "ray_sens")

        m = np.empty((3,) + tuple(self.shape)) if maps else None
        if not rows:
            call(m, None, 0, (None, None, None, None))
            return m, None, status
        row_ptr = np.zeros(n + 1, dtype=np.int64)
        call(None, row_ptr, 0, (None, None, None, None))  # the count pass
        cap = int(row_ptr[n])
        arrays = (np.empty(cap, dtype=np.int32), np.empty(cap), np.empty(cap), np.empty(cap))
        call(m, row_ptr, cap, arrays)
        return m, (row_ptr,) + arrays, status

    SOLVE_REASONS = ("tol", "max_iter", "breakdown")

    def sens_op_build(self, ray_len, ray_xy=None, subgrid=1, flags=None, quantity=1, col_scale=None):
        """Build and keep on the device the operator A (nrays x nnz*nnx) of one quantity of the rays'
        sensitivities (alifmm_sens_op_build): quantity 0 len, 1 time, 2 dth; col_scale (nnz, nnx)
        scales the columns (0 freezes a cell).  The request is ray_sens's.  Returns (entries,
        status)."""
        lens = _ci32(np.atleast_1d(ray_len))
        n = len(lens)
        xy = None
        if ray_xy is not None:
            xy = _c64(ray_xy).reshape(-1, 2)
            if len(xy) != int(np.maximum(lens, 0).sum(dtype=np.int64)):
                raise ValueError("ray_xy holds %d points, ray_len adds up to %d"
                                 % (len(xy), int(np.maximum(lens, 0).sum(dtype=np.int64))))
        fl = None if flags is None else _ci32(np.atleast_1d(flags))
        if fl is not None and len(fl) != n:
            raise ValueError("flags must have one value per ray")
        cs = None
        if col_scale is not None:
            cs = _c64(col_scale)
            if cs.size != int(np.prod(self.shape)):
                raise ValueError("col_scale must have one value per cell of the model")
        status = np.zeros(n, dtype=np.int32)
        entries = ctypes.c_int64(0)
        self._chk(lib().alifmm_sens_op_build(self._h, int(subgrid), n, _ptr(lens), _ptr(fl), _ptr(xy), int(quantity),
                                             _ptr(cs), ctypes.addressof(entries), _ptr(status)), "sens_op_build")
        self._op_rays = n
        return entries.value, status

    def sens_op_apply(self, v, transpose=False):
        """A v (v one value per cell; returns one per ray), or with transpose Aᵀ v (v one value per
        ray; returns (nnz, nnx)), by the resident operator.  Bit-reproducible."""
        nrays, ncell = getattr(self, "_op_rays", 0), int(np.prod(self.shape))
        v = _c64(v).ravel()
        if len(v) != (nrays if transpose else ncell):
            raise ValueError("the vector has %d values, the operator wants %d" % (len(v), nrays if transpose else ncell))
        out = np.zeros(ncell if transpose else nrays)
        self._chk(lib().alifmm_sens_op_apply(self._h, int(bool(transpose)), _ptr(v), _ptr(out)), "sens_op_apply")
        return out.reshape(self.shape) if transpose else out

    def sens_op_solve(self, rhs, damp=0.0, smooth=0.0, max_iter=50, tol=1e-6):
        """CGLS on min |A x - rhs|² + damp² |x|² + smooth² |D x|² from x = 0 with the resident operator
        (alifmm_sens_op_solve).  Returns (x (nnz, nnx), info): info = dict(iterations, grad0, grad,
        rhs_norm, res_norm, reason ("tol", "max_iter" or "breakdown"), entries)."""
        rhs = _c64(rhs).ravel()
        if len(rhs) != getattr(self, "_op_rays", 0):
            raise ValueError("rhs has %d values, the operator has %d rays" % (len(rhs), getattr(self, "_op_rays", 0)))
        x = np.zeros(self.shape)
        info = np.zeros(8)
        self._chk(lib().alifmm_sens_op_solve(self._h, _ptr(rhs), float(damp), float(smooth), int(max_iter), float(tol),
                                             _ptr(x), _ptr(info)), "sens_op_solve")
        return x, {"iterations": int(info[0]), "grad0": info[1], "grad": info[2], "rhs_norm": info[3],
                   "res_norm": info[4], "reason": self.SOLVE_REASONS[int(info[5])], "entries": int(info[6])}

    def sens_op_release(self):
        self._chk(lib().alifmm_sens_op_release(self._h), "sens_op_release")

    def source_stats(self, slot):
        steps = np.zeros(4, dtype=np.int64)
        sw = ctypes.c_int64(0)
        self._chk(lib().alifmm_source_stats(self._h, int(slot), _ptr(steps), ctypes.byref(sw)), "source_stats")
        return steps, sw.value

    def band_profile(self, slot):
        out = np.zeros(14, dtype=np.int64)
        self._chk(lib().alifmm_band_profile(self._h, int(slot), _ptr(out)), "band_profile")
        return out

    def band_span(self, slot):
        """(start, end) wall clock [100 MHz ticks] of the band kernel's member 0 for a slot's source."""
        out = np.zeros(2, dtype=np.int64)
        self._chk(lib().alifmm_band_span(self._h, int(slot), _ptr(out)), "band_span")
        return int(out[0]), int(out[1])

    def init_profile(self, i):
        """Source-init profile of source i of the last chunk: ticks (100 MHz) of stage 1/2/3 and the
        exact prefix, their pops, relax-role busy ticks, relaxations | fallbacks << 32
        (alifmm_init_profile)."""
        out = np.zeros(16, dtype=np.int64)
        self._chk(lib().alifmm_init_profile(self._h, int(i), _ptr(out)), "init_profile")
        return out

    def last_timing(self):
        a, b, c = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        self._chk(lib().alifmm_last_timing(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
                  "last_timing")
        return a.value, b.value, c.value

    def time_between_points(self, x1, x2, y1, y2, subgrid):
        x1, x2, y1, y2 = (_c64(np.atleast_1d(v)) for v in (x1, x2, y1, y2))
        out = np.empty(len(x1))
        self._chk(lib().alifmm_time_between_points(self._h, len(x1), _ptr(x1), _ptr(x2), _ptr(y1), _ptr(y2),
                                                   int(subgrid), _ptr(out)), "time_between_points")
        return out

    def local_ops(self, op, ttn, nsts, iz, ix, dnx, dnz, nnz_arg, nnx_arg, cveln, cvelpn, cvm, cstif, tab):
        """Batched update() (op 0) / fouds18_A() (op 1) on (n, pz, px) patches.  Test entries, same
        inputs and bits (include/alifmm.h): op 3 update() on the kernels' register neighbourhood,
        op 4 the same selected over a wavefront, op 5 fouds18_A() on four lanes per case."""
        ttn = _c64(ttn)
        n, pz, px = ttn.shape
        nsts = _ci32(nsts)
        out = np.empty(n)
        tab = _c64(tab)
        cst = None if cstif is None else _ci64(cstif).reshape(n, 5)
        args = [_ci32(iz), _ci32(ix), _c64(dnx), _c64(dnz), _ci32(nnz_arg), _ci32(nnx_arg), _c64(cveln),
                _ci64(cvelpn), _c64(cvm)]
        self._chk(lib().alifmm_local_ops(self._h, int(op), n, pz, px, _ptr(ttn), _ptr(nsts), *[_ptr(a) for a in args],
                                         _ptr(cst), _ptr(tab), tab.shape[1], _ptr(out)), "local_ops")
        return out

    CR_FN = {"atan": 0, "sin": 1, "cos": 2, "tan": 3, "sincos": 4}

    def cr_math(self, fn, x, lds_tables=False):
        """The device's correctly rounded atan / sin / cos / tan / sincos (csrc/cr_math.h) of every
        element of x (alifmm_cr_math); fn: a name of CR_FN or its number.  One array of x's shape,
        a (sin, cos) pair for sincos.  lds_tables: read the tables from LDS, as the solver kernels do."""
        if isinstance(fn, str):
            if fn not in self.CR_FN:
                raise AlifmmError("cr_math: unknown function %r (one of %s)" % (fn, ", ".join(self.CR_FN)))
            fn = self.CR_FN[fn]
        x = _c64(x)
        out = np.empty_like(x)
        out2 = np.empty_like(x) if fn == 4 else None
        self._chk(lib().alifmm_cr_math(self._h, int(fn), int(lds_tables), x.size, _ptr(x), _ptr(out), _ptr(out2)),
                  "cr_math")
        return (out, out2) if fn == 4 else out

    def fouds18_band(self, ttn, nsts, iz, ix, dnx, dnz, nnz_arg, nnx_arg, mz, mx, quant=0, lanes=False):
        """fouds18_A() as the band kernel evaluates it: material of resident-model cell (mz, mx)
        through the per-material record and precomputed slownesses (alifmm_fouds18_band).
        lanes: on four lanes per case, as the kernel's fallback rounds (alifmm_fouds18_band_lanes)."""
        ttn = _c64(ttn)
        n, pz, px = ttn.shape
        out = np.empty(n)
        nsts = _ci32(nsts)
        args = [_ci32(iz), _ci32(ix), _c64(dnx), _c64(dnz), _ci32(nnz_arg), _ci32(nnx_arg), _ci32(mz), _ci32(mx)]
        fn = lib().alifmm_fouds18_band_lanes if lanes else lib().alifmm_fouds18_band
        self._chk(fn(self._h, n, pz, px, _ptr(ttn), _ptr(nsts), *[_ptr(a) for a in args], int(quant), _ptr(out)),
                  "fouds18_band")
        return out


class Comm:
    """RCCL communicator over contexts on distinct GPUs (include/alifmm.h alifmm_comm_*): gathers
    resident fields onto one GPU over xGMI.  Comm.all(ctxs): one process driving every context;
    Comm.rank(ctx, nranks, rank, uid): one process per GPU, uid = Comm.unique_id() made by one rank
    and shared by the caller (e.g. torch.distributed.broadcast_object_list)."""

    def __init__(self, handle, ctxs):
        self._h = handle
        self.ctxs = list(ctxs)
        _live.add(self)

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        if lib().alifmm_comm_unique_id(buf) != 0:
            raise AlifmmError("alifmm_comm_unique_id failed (RCCL unavailable)")
        return buf.raw

    @classmethod
    def all(cls, ctxs):
        arr = (ctypes.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
        h = ctypes.c_void_p()
        ctxs[0]._chk(lib().alifmm_comm_init_all(arr, len(ctxs), ctypes.byref(h)), "comm_init_all")
        return cls(h, ctxs)

    @classmethod
    def rank(cls, ctx, nranks, rank, uid):
        if len(uid) != 128:
            raise ValueError("RCCL unique id must be 128 bytes")
        h = ctypes.c_void_p()
        ctx._chk(lib().alifmm_comm_init_rank(ctx._h, int(nranks), int(rank), ctypes.create_string_buffer(uid, 128),
                                             ctypes.byref(h)), "comm_init_rank")
        return cls(h, [ctx])

    def gather(self, root, subgrid, first_slot, count, dst_slot=0):
        """Rank r's slots first_slot[r] .. +count[r]-1 -> the root's slots dst_slot + sum(count[:r]) + i.
        Every rank passes the same lists.  Returns the wall time [ms]."""
        fs = np.ascontiguousarray(first_slot, dtype=np.int32)
        cn = np.ascontiguousarray(count, dtype=np.int32)
        ms = ctypes.c_double(0)
        rc = lib().alifmm_gather_fields(self._h, int(root), int(subgrid), _ptr(fs), _ptr(cn), int(dst_slot),
                                        ctypes.byref(ms))
        if rc != 0:
            msg = lib().alifmm_comm_last_error(self._h)
            raise AlifmmError("gather_fields failed (rc=%d): %s" % (rc, msg.decode() if msg else ""))
        return ms.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value and _lib is not None:
            _lib.alifmm_comm_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gather_layout(counts):
    """Root slot offset of every rank's first field in alifmm_gather_fields (rank order)."""
    return np.concatenate(([0], np.cumsum(np.asarray(counts, dtype=np.int64))))[:-1]


def bandpass_response(nfft, fs, f_lo, f_hi, taper=None):
    """A real band-pass response for Context.trace_spectral: (nfft,) float64 in numpy.fft's bin
    order, 1 for f_lo <= |f| <= f_hi, raised-cosine edges of width taper outside them
    (0.5 (1 - cos(pi (|f| - f_lo + taper) / taper)) below f_lo, mirrored above f_hi), 0 beyond; the
    same on positive and negative frequencies, so a real trace stays real.  Host numpy.

    fs: the sampling rate; 0 <= f_lo < f_hi <= fs / 2; taper >= 0 in the same unit (None: a quarter
    of the band's width; 0: a brick wall)."""
    nfft, fs, f_lo, f_hi = int(nfft), float(fs), float(f_lo), float(f_hi)
    if nfft < 1:
        raise ValueError("bandpass_response: nfft %d" % nfft)
    if not (fs > 0 and np.isfinite(fs)):
        raise ValueError("bandpass_response: fs %g" % fs)
    if not 0 <= f_lo < f_hi <= fs / 2:
        raise ValueError("bandpass_response: band edges (%g, %g) are not 0 <= f_lo < f_hi <= fs / 2 = %g"
                         % (f_lo, f_hi, fs / 2))
    taper = (f_hi - f_lo) / 4 if taper is None else float(taper)
    if not (taper >= 0 and np.isfinite(taper)):
        raise ValueError("bandpass_response: taper %g" % taper)
    f = np.abs(np.fft.fftfreq(nfft, 1.0 / fs))
    h = ((f >= f_lo) & (f <= f_hi)).astype(np.float64)
    if taper > 0:
        lo = (f < f_lo) & (f > f_lo - taper)
        hi = (f > f_hi) & (f < f_hi + taper)
        h[lo] = 0.5 * (1 - np.cos(np.pi * (f[lo] - f_lo + taper) / taper))
        h[hi] = 0.5 * (1 - np.cos(np.pi * (f_hi + taper - f[hi]) / taper))
    return h


def matched_response(nfft, pulse, origin=0):
    """The matched filter of a pulse as a response for Context.trace_spectral and trace_pick:
    (nfft,) complex128 in numpy.fft's bin order, the frequency response of correlation with the
    pulse, out[t] = sum_j conj(pulse[j]) in[t + j - origin] (Context.trace_fir(..., transpose=True),
    circular over nfft points), divided by sum |pulse|^2, so an echo that is the pulse itself, its
    time zero on sample n, peaks on sample n with the echo's amplitude.  Multiply it with
    bandpass_response() to do both in one pass.  Host numpy.

    The filter is circular: the output equals trace_fir's wherever no tap reaches over an end of
    the nfft points, everywhere when nfft >= nt + ntap - 1 (the padding holds what wraps).
    pulse: 1-D real or complex, 1 <= ntap <= nfft, finite, not all zero; origin: the tap index of
    its time zero, 0 <= origin < ntap."""
    nfft, origin = int(nfft), int(origin)
    h = np.asarray(pulse)
    if h.ndim != 1 or not 1 <= h.shape[0] <= nfft:
        raise ValueError("matched_response: pulse must be 1-D with 1 .. nfft = %d taps, not %s" % (nfft, h.shape))
    if not 0 <= origin < h.shape[0]:
        raise ValueError("matched_response: origin %d outside [0, %d)" % (origin, h.shape[0]))
    h = h.astype(np.complex128)
    norm = float(np.sum(h.real ** 2 + h.imag ** 2))
    if not (np.isfinite(norm) and norm > 0):
        raise ValueError("matched_response: the pulse must be finite and not all zero")
    g = np.zeros(nfft, dtype=np.complex128)  # the impulse response: conj(pulse[j]) at delay origin - j
    np.add.at(g, (origin - np.arange(h.shape[0])) % nfft, np.conj(h))
    return np.fft.fft(g) / norm


def pick_gates(around, half_width, t0, fs, nt):
    """The gates of ALI_FMM.pick_times: per entry of `around` (predicted times, any shape) the
    samples n of a trace of nt samples, sample n at time t0 + n / fs, with
    ceil((around - half_width - t0) fs) <= n <= floor((around + half_width - t0) fs), clipped to
    0 .. nt - 1.  Returns (lo, hi) int32 of around's shape, the gate being lo <= n < hi; lo = hi = 0
    where around is NaN or infinite or no sample of the trace lies inside."""
    around = np.asarray(around, dtype=np.float64)
    half_width, t0, fs, nt = float(half_width), float(t0), float(fs), int(nt)
    if not (half_width >= 0 and np.isfinite(half_width)):
        raise ValueError("pick_gates: half_width %g" % half_width)
    if not (fs > 0 and np.isfinite(fs)) or not np.isfinite(t0):
        raise ValueError("pick_gates: fs %g, t0 %g" % (fs, t0))
    if nt < 1:
        raise ValueError("pick_gates: nt %d" % nt)
    ok = np.isfinite(around)
    a = np.where(ok, around, 0.0)
    first = np.maximum(np.ceil((a - half_width - t0) * fs), 0.0)
    last = np.minimum(np.floor((a + half_width - t0) * fs), nt - 1.0)
    ok &= first <= last
    lo = np.where(ok, first, 0.0).astype(np.int32)
    hi = np.where(ok, last + 1.0, 0.0).astype(np.int32)
    return lo, hi


_default = {}


def default_context(device=0):
    """Process-wide context per device (created on first use)."""
    with _lock:
        ctx = _default.get(device)
    if ctx is None:
        ctx = Context(device)
        with _lock:
            _default[device] = ctx
    return ctx
