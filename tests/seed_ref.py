"""alifmm_travel_seeded (include/alifmm.h) restated on the CPU: the contract in Python.

Step -1 and the band run of oracle/band_model.c band_run (sweeps 1), Jacobi-style, with the status
codes the device shares (-1 far, -3 far and claimed, 0 known, 1 close, 2 close and claimed) and far
cells holding ttn 0.  The local operators are the oracle library's (oref_update, and where it
returns -1 oref_fouds18), called on one persistent model and state.  TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

import oracle as O


class SeedRef:
    def __init__(self, veln, velpn, vel_map, stif_den, table, dnx, dnz=None):
        self.m = O._Model(veln, velpn, vel_map, stif_den, table, table)
        self.dnx, self.dnz = float(dnx), float(dnx if dnz is None else dnz)
        self.nz, self.nx = self.m.nnz, self.m.nnx
        self.L = O.lib()

    def _evaluate(self, cells, ttn, nsts):
        m, p, nz, nx = self.m, O._ptr, self.nz, self.nx
        mat = (p(m.veln), p(m.velpn), p(m.vel_map), p(m.stif))
        out = []
        for r in cells:
            z, x = divmod(int(r), nx)
            v = self.L.oref_update(nz, nx, p(ttn), p(nsts), z, x, self.dnx, nz, nx, *mat, p(m.ph), m.ncol)
            if v == -1.0:
                v = self.L.oref_fouds18(nz, nx, p(ttn), p(nsts), z, x, self.dnx, self.dnz, *mat, p(m.av), m.ncol)
            out.append(v)
        return out

    def _claim(self, accepted, nsts):
        """Non-known in-grid 4-neighbours of the accepted cells (x - 1, x + 1, z - 1, z + 1), each once."""
        nz, nx, C = self.nz, self.nx, []
        for idx in accepted:
            z, x = divmod(int(idx), nx)
            for zz, xx in ((z, x - 1), (z, x + 1), (z - 1, x), (z + 1, x)):
                if 0 <= zz < nz and 0 <= xx < nx:
                    r = zz * nx + xx
                    if nsts[r] == -1 or nsts[r] == 1:
                        nsts[r] = -3 if nsts[r] == -1 else 2
                        C.append(r)
        return C

    def field(self, seed_iz, seed_ix, seed_t, vmax, cdelta, r0, cdelta_far=0.0, r_far=0.0):
        """The field from seeds (seed_iz[k], seed_ix[k]) with times seed_t[k]; band options as read
        back from a context (the widths in force)."""
        nz, nx = self.nz, self.nx
        ttn, nsts = np.zeros(nz * nx), np.full(nz * nx, -1, dtype=np.int32)
        seeds = np.asarray(seed_iz, dtype=np.int64) * nx + np.asarray(seed_ix, dtype=np.int64)
        ttn[seeds], nsts[seeds] = np.asarray(seed_t, dtype=np.float64), 0
        delta, t0 = cdelta * self.dnx / vmax, r0 * self.dnx / vmax
        delta_far = cdelta_far * self.dnx / vmax
        tfar = r_far * self.dnx / vmax if r_far > 0 and cdelta_far > 0 else 0.0
        # step -1: the seeds are the accepted set; the close cells in ascending cell index
        L = sorted(self._claim(seeds, nsts))
        ttn[L], nsts[L] = self._evaluate(L, ttn, nsts), 1
        while L:
            La = np.asarray(L, dtype=np.int64)
            tl = ttn[La]
            tmin = float(tl.min())
            dl = delta
            if t0 > 0 and tmin < t0:
                dl = delta * (tmin / t0)
            if tfar > 0 and tmin > tfar:
                dl = delta + (delta_far - delta) * min(1.0, (tmin - tfar) / tfar)
            acc = tl <= tmin + dl
            nsts[La[acc]] = 0
            L = [int(v) for v in La[~acc]]
            C = self._claim(La[acc], nsts)
            V = self._evaluate(C, ttn, nsts)
            for r, v in zip(C, V):
                ttn[r] = v
                if nsts[r] == -3:
                    L.append(r)
                nsts[r] = 1
        return ttn.reshape(nz, nx)

    def field_c(self, seed_iz, seed_ix, seed_t, vmax, cdelta, r0, cdelta_far=0.0, r_far=0.0, lib=None, log=False):
        """field() by oracle/band_model.c oband_seeded: the same statement in C, for lists of thousands
        of cells (tests/test_long_cases_ref.py holds the two bit-equal).  lib: a build from
        oracle.open_lib (the correctly rounded one); log: also the run's oracle.BandLog."""
        seeds = np.asarray(seed_iz, dtype=np.int64) * self.nx + np.asarray(seed_ix, dtype=np.int64)
        run = lambda: O.band_seeded(self.m, seeds, seed_t, self.dnx, self.dnz, vmax, cdelta, r0, cdelta_far,  # noqa: E731
                                    r_far, lib=lib)[0]
        if not log:
            return run()
        return O.band_logged(run, self.nz * self.nx, lib=lib)
