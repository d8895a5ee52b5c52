/*
 * oracle/band_model.c — TEST INFRASTRUCTURE ONLY.
 *
 * CPU model of the MI355X formulation (band-synchronous "Delta-stepping" FMM):
 * every step accepts ALL close cells with T <= Tmin + delta, then re-evaluates the reference's
 * local operator (update(), fouds18_A() fallback) for their non-known 4-neighbours Jacobi-style
 * against the post-acceptance state, exactly as csrc/fmm_band.hip does.  It reuses the oracle's
 * restated local operators, so GPU-vs-model differences isolate device arithmetic, and
 * model-vs-oracle differences isolate the reformulation.  Used by tests/ only.
 */
#include "alifmm_oracle.c"

/* status codes shared with the device kernel */
enum { S_FAR = -1, S_FARC = -3, S_KNOWN = 0, S_CLOSE = 1, S_CLOSEC = 2 };

typedef struct {
    fstate_t f;        /* ttn + nsts (nsts holds the status codes above) */
    int32_t *L, *L2, *A, *C;
    int32_t *accstep;  /* step at which a cell was accepted (stage-1 quirk test) */
    double *V;
    long nL;
} bstate_t;

static int bstate_alloc(bstate_t *b, int nz, int nx, double *ttn_ext) {
    if (fstate_alloc(&b->f, nz, nx, 4, ttn_ext)) return -1;
    size_t n = (size_t)nz * nx;
    b->L = (int32_t *)malloc(n * 4);
    b->L2 = (int32_t *)malloc(n * 4);
    b->A = (int32_t *)malloc(n * 4);
    b->C = (int32_t *)malloc(n * 4);
    b->accstep = (int32_t *)malloc(n * 4);
    b->V = (double *)malloc(n * 8);
    b->nL = 0;
    if (!b->L || !b->L2 || !b->A || !b->C || !b->accstep || !b->V) return -1;
    for (size_t i = 0; i < n; i++) b->accstep[i] = -1;
    return 0;
}
static void bstate_free(bstate_t *b, int own) {
    fstate_free(&b->f, own);
    free(b->L); free(b->L2); free(b->A); free(b->C); free(b->accstep); free(b->V);
}
static inline void push_close(bstate_t *b, long idx) {
    /* the heap's "addtree": status close + list entry (duplicates are harmless: see dedupe) */
    if (b->f.nsts[idx] != S_CLOSE) { b->f.nsts[idx] = S_CLOSE; b->L[b->nL++] = (int32_t)idx; }
}

/* optional wider band far from the source on the main grid (the device option cdelta_far / r_far,
   fmm_band_k.hip): past tfar the width ramps from delta to delta_far over tfar .. 2 tfar */
static double g_cdelta_far = 0.0, g_r_far = 0.0;
void oband_set_far(double cdelta_far, double r_far) { g_cdelta_far = cdelta_far; g_r_far = r_far; }

/* optional record of the main grid's band run, for the list census of tests/long_cases.py: the
   step at which each cell was accepted (acc[cell], the caller's fill elsewhere), and one entry per
   close-list insertion and per evaluation: (cell, step, flag), flag bit 0: the cell was far (it
   joins the close list), bit 1: update() returned -1 (fouds18_A() ran).  Step -1 holds the hand-over
   (the initial close list; in a seeded run its evaluations).  Between oband_log_begin and
   oband_log_end (the entry count, or -1 when cap was too small) on one thread. */
static struct { int32_t *acc, *cell, *step; int8_t *flag; long cap, n; int on; } g_log;
void oband_log_begin(int32_t *acc, int32_t *cell, int32_t *step, int8_t *flag, long cap) {
    g_log.acc = acc; g_log.cell = cell; g_log.step = step; g_log.flag = flag; g_log.cap = cap; g_log.n = 0;
    g_log.on = 1;
}
long oband_log_end(void) { g_log.on = 0; return g_log.n <= g_log.cap ? g_log.n : -1; }
static inline void log_entry(long cell, long step, int flag) {
    if (g_log.n < g_log.cap) {
        g_log.cell[g_log.n] = (int32_t)cell; g_log.step[g_log.n] = (int32_t)step; g_log.flag[g_log.n] = (int8_t)flag;
    }
    g_log.n++;
}

/* one band run on a grid until the close list drains (main) or the window edge is hit (stages) */
static long band_run(bstate_t *b, const mat_t *m, const loopcfg_t *c, double delta, int sweeps, double t0,
                     double delta_far, double tfar) {
    fstate_t *f = &b->f;
    long nx = f->nnx, nz = f->nnz;
    long steps = 0;
    int finished = 0;
    const int lg = g_log.on && !c->stage;
    while (b->nL > 0 && !finished) {
        double tmin = INFINITY;
        for (long e = 0; e < b->nL; e++) { double t = f->ttn[b->L[e]]; if (t < tmin) tmin = t; }
        /* near-source schedule: the band narrows in proportion to Tmin while Tmin < t0 */
        double dl = delta;
        if (t0 > 0 && tmin < t0) dl = delta * (tmin / t0);
        if (tfar > 0 && tmin > tfar) dl = delta + (delta_far - delta) * fmin(1.0, (tmin - tfar) / tfar);
        double thr = tmin + dl;
        long nA = 0, nL2 = 0;
        for (long e = 0; e < b->nL; e++) {
            long idx = b->L[e];
            if (f->ttn[idx] <= thr) {
                f->nsts[idx] = S_KNOWN;
                b->accstep[idx] = (int32_t)steps;
                if (lg) g_log.acc[idx] = (int32_t)steps;
                b->A[nA++] = (int32_t)idx;
            } else {
                b->L2[nL2++] = (int32_t)idx;
            }
        }
        /* neighbours are visited in the reference's order (x-1, x+1, z-1, z+1; :2065-2102).  seq=1:
           one sub-phase per direction, each committed before the next, so an update sees the
           values its siblings of the same pop received earlier (sequential semantics for one pop);
           seq=0: all four directions evaluated Jacobi-style against the post-acceptance state. */
        int ndirph = sweeps >= 10 ? 4 : 1;
        for (int ph = 0; ph < ndirph; ph++) {
            long nC = 0;
            for (long a = 0; a < nA; a++) {
                long idx = b->A[a], iz = idx / nx, ix = idx % nx;
                long nb[4][2] = {{iz, ix - 1}, {iz, ix + 1}, {iz - 1, ix}, {iz + 1, ix}};
                for (int q = 0; q < 4; q++) {
                    if (ndirph == 4 && q != ph) continue;
                    long z = nb[q][0], x = nb[q][1];
                    if (z < 0 || z >= nz || x < 0 || x >= nx) {
                        if (c->stage) {
                            if (q < 2 && labs(c->isx_s - x) == c->max_dist + 1) finished = 1;
                            if (q >= 2 && labs(c->isz_s - z) == c->max_dist + 1) finished = 1;
                        }
                        continue;
                    }
                    long r = z * nx + x;
                    int32_t s = f->nsts[r];
                    if (b->accstep[r] == -2 - (int32_t)steps) continue; /* already updated this step */
                    if (s == S_FAR) { f->nsts[r] = S_FARC; b->C[nC++] = (int32_t)r; }
                    else if (s == S_CLOSE) { f->nsts[r] = S_CLOSEC; b->C[nC++] = (int32_t)r; }
                }
            }
            for (long k = 0; k < nC; k++) {
                long r = b->C[k], iz = r / nx, ix = r % nx;
                int quirk = 0;
                if (c->quirk_nnz && f->nsts[r] == S_CLOSEC) {
                    if ((ix > 0 && b->accstep[r - 1] == steps) || (ix < nx - 1 && b->accstep[r + 1] == steps)) quirk = 1;
                }
                double v = oref_update_f(f, m, c->ph, iz, ix, c->dnx, quirk ? nx : nz, nx);
                if (lg) log_entry(r, steps, (f->nsts[r] == S_FARC ? 1 : 0) | (v == -1.0 ? 2 : 0));
                if (v == -1.0) v = oref_fouds18_f(f, m, c->av, iz, ix, c->dnx, c->dnz_fouds, nx, nz);
                b->V[k] = v;
            }
            for (long k = 0; k < nC; k++) {
                long r = b->C[k];
                f->ttn[r] = b->V[k];
                if (f->nsts[r] == S_FARC) b->L2[nL2++] = (int32_t)r;
                f->nsts[r] = S_CLOSE;
                if (ndirph == 4 && b->accstep[r] < 0) b->accstep[r] = -2 - (int32_t)steps;
            }
        }
        int32_t *t = b->L; b->L = b->L2; b->L2 = t;
        b->nL = nL2;
        steps++;
    }
    return steps;
}

/* hand-over (reference :2006-2040 etc.) into a band state */
static void band_handover(const fstate_t *s, long isz_s, long isx_s, bstate_t *d, long isz_d, long isx_d) {
    for (long i = 0; i < s->nnz + 1; i += 3) {
        for (long j = 0; j < s->nnx + 1; j += 3) {
            long pz = isz_d + (i - isz_s) / 3, px = isx_d + (j - isx_s) / 3;
            long di = pz * d->f.nnx + px;
            d->f.ttn[di] = s->ttn[i * s->nnx + j];
            int32_t st = s->nsts[i * s->nnx + j];
            if (st == 0) {
                d->f.nsts[di] = S_KNOWN;
                int outer = 0;
                if (i - 3 >= 0) { if (s->nsts[(i - 3) * s->nnx + j] == -1) outer = 1; } else outer = 1;
                if (i + 3 <= s->nnz - 1) { if (s->nsts[(i + 3) * s->nnx + j] == -1) outer = 1; } else outer = 1;
                if (j - 3 >= 0) { if (s->nsts[i * s->nnx + j - 3] == -1) outer = 1; } else outer = 1;
                if (j + 3 <= s->nnx - 1) { if (s->nsts[i * s->nnx + j + 3] == -1) outer = 1; } else outer = 1;
                if (outer) push_close(d, di);
            }
            if (st > 0) push_close(d, di);
        }
    }
}

/* travel() with band stages (exact_init=0) or the reference's heap stages (exact_init=1) */
int oband_travel(double scx, double scz, int nnz, int nnx, const double *veln, const int64_t *velpn,
                 const double *vel_map, const int64_t *stif, const double *av_, const double *ph_, int ncol,
                 double gox, double goz, double dnx, double dnz, double cdelta, double vmax, int exact_init,
                 int sweeps, double r0, double exact_r, double *ttn, long *steps_out) {
    base_t bb;
    if (make_base(&bb, nnz, nnx, veln, velpn, vel_map, stif)) return -1;
    const mat_t *base = &bb.m;
    table_t tav = {av_, ncol}, tph = {ph_, ncol};
    const table_t *av = &tav, *ph = &tph;
    memset(ttn, 0, sizeof(double) * (size_t)nnz * nnx);
    long isx = pyround((scx - gox) / dnx), isz = pyround((scz - goz) / dnz);
    long steps[4] = {0, 0, 0, 0};
    long sgs[3] = {27, 9, 3}, sizes[3] = {2, 6, 13};
    fstate_t prev;       /* previous stage (heap or band) in fstate form */
    fstate_t hprev_keep; /* stage-3 heap state for the exact main-loop prefix */
    bstate_t bprev;
    int have_b = 0;
    long pisz = 0, pisx = 0;
    view_t views[3];
    for (int st = 0; st < 3; st++) {
        long sg = sgs[st], size = sizes[st];
        long left = imax(0, isx - size), right = imin(nnx - 1, isx + size);
        long bottom = imax(0, isz - size), top = imin(nnz - 1, isz + size);
        make_view(&views[st], base, bottom, top, left, right, sg);
        long isx_s = sg * (isx - left), isz_s = sg * (isz - bottom);
        double dn = dnx / sg;
        loopcfg_t c = {av, ph, dn, dn, 1, (int)isx_s, (int)isz_s, (int)(sg * size), st == 0, 0.0};
        if (exact_init == 1 || (exact_init == 2 && st == 0) || (exact_init == 3 && st < 2)) {
            fstate_t f;
            fstate_alloc(&f, views[st].m.nnz, views[st].m.nnx, 0, NULL);
            if (st == 0) {
                straight_rays(&f, isz_s, isx_s, (sg - 1) / 2, dn, base, (int)isz, (int)isx, av, 0);
                add_edges(&f, isz_s, isx_s, (sg - 1) / 2);
            } else {
                handover(&prev, pisz, pisx, &f, isz_s, isx_s);
                fstate_free(&prev, 1);
            }
            fmm_loop(&f, &views[st].m, &c);
            prev = f;
            have_b = 0;
            if (st == 2 && exact_r > 0) {
                fstate_alloc(&hprev_keep, f.nnz, f.nnx, 0, NULL);
                memcpy(hprev_keep.ttn, f.ttn, sizeof(double) * (size_t)f.nnz * f.nnx);
                memcpy(hprev_keep.nsts, f.nsts, sizeof(int32_t) * (size_t)f.nnz * f.nnx);
            }
        } else {
            bstate_t b;
            bstate_alloc(&b, views[st].m.nnz, views[st].m.nnx, NULL);
            if (st == 0) {
                straight_rays(&b.f, isz_s, isx_s, (sg - 1) / 2, dn, base, (int)isz, (int)isx, av, 0);
                /* add_edges: the window border of the straight-ray square becomes close */
                long s1 = (sg - 1) / 2, n1z = b.f.nnz, n1x = b.f.nnx;
                if (isz_s - s1 >= 0) for (long i = imax(0, isx_s - s1); i <= imin(n1x - 1, isx_s + s1); i++) push_close(&b, (isz_s - s1) * n1x + i);
                if (isz_s + s1 <= n1z - 1) for (long i = imax(0, isx_s - s1); i <= imin(n1x - 1, isx_s + s1); i++) push_close(&b, (isz_s + s1) * n1x + i);
                if (isx_s - s1 >= 0) for (long i = imax(0, isz_s - s1); i <= imin(n1z - 1, isz_s + s1); i++) push_close(&b, i * n1x + isx_s - s1);
                if (isx_s + s1 <= n1x - 1) for (long i = imax(0, isz_s - s1); i <= imin(n1z - 1, isz_s + s1); i++) push_close(&b, i * n1x + isx_s + s1);
            } else if (!have_b) {
                band_handover(&prev, pisz, pisx, &b, isz_s, isx_s);
                fstate_free(&prev, 1);
            } else {
                band_handover(&bprev.f, pisz, pisx, &b, isz_s, isx_s);
                /* map band status back to heap-style codes for the hand-over test (close > 0) */
                bstate_free(&bprev, 1);
            }
            steps[st] = band_run(&b, &views[st].m, &c, cdelta * dn / vmax, sweeps, r0 * dnx / vmax, 0.0, 0.0);
            bprev = b;
            have_b = 1;
        }
        pisz = isz_s; pisx = isx_s;
    }
    loopcfg_t c = {av, ph, dnx, dnz, 0, 0, 0, 0, 0, 0.0};
    bstate_t bm;
    bstate_alloc(&bm, nnz, nnx, ttn);
    if (!have_b) { band_handover(&prev, pisz, pisx, &bm, isz, isx); fstate_free(&prev, 1); }
    else { band_handover(&bprev.f, pisz, pisx, &bm, isz, isx); bstate_free(&bprev, 1); }
    if (exact_r > 0) {
        /* exact heap-ordered prefix of the main loop (the reference's own pop order near the source),
           then the band continues from the heap's state (close = in heap, known, far) */
        fstate_t h;
        fstate_alloc(&h, (int)nnz, (int)nnx, 0, ttn);
        for (long i = 0; i < (long)nnz * nnx; i++) h.nsts[i] = -1;
        /* rebuild the reference hand-over into the heap (row-major addtree order) */
        memset(ttn, 0, sizeof(double) * (size_t)nnz * nnx);
        if (have_b) { fprintf(stderr, "exact_r needs band stages off\n"); }
        handover(&hprev_keep, pisz, pisx, &h, isz, isx);
        loopcfg_t ce = c;
        ce.tstop = exact_r * dnx / vmax;
        fmm_loop(&h, base, &ce);
        for (long i = 0; i < (long)nnz * nnx; i++) bm.f.nsts[i] = -1;
        bm.nL = 0;
        for (long i = 0; i < (long)nnz * nnx; i++) {
            if (h.nsts[i] == 0) bm.f.nsts[i] = S_KNOWN;
            else if (h.nsts[i] > 0) push_close(&bm, i);
        }
        fstate_free(&h, 0);
        fstate_free(&hprev_keep, 1);
    }
    if (g_log.on) for (long e = 0; e < bm.nL; e++) log_entry(bm.L[e], -1, 1);
    steps[3] = band_run(&bm, base, &c, cdelta * dnx / vmax, sweeps, r0 * dnx / vmax, g_cdelta_far * dnx / vmax,
                        g_r_far > 0 && g_cdelta_far > 0 ? g_r_far * dnx / vmax : 0.0);
    bstate_free(&bm, 0);
    for (int st = 0; st < 3; st++) free_view(&views[st]);
    free_base(&bb);
    if (steps_out) for (int i = 0; i < 4; i++) steps_out[i] = steps[i];
    (void)have_b;
    return 0;
}

/* alifmm_travel_seeded (include/alifmm.h) as tests/seed_ref.py SeedRef.field states it, in C for the
 * long lists of tests/long_cases.py: the seeds are known with their times; step -1 evaluates their far
 * in-grid 4-neighbours in ascending cell order, Jacobi-style, and makes them close; the band runs
 * from there (band_run, sweeps 1).  cdelta / cdelta_far: the widths in force. */
static int cmp_i32(const void *a, const void *b) {
    int32_t x = *(const int32_t *)a, y = *(const int32_t *)b;
    return x < y ? -1 : x > y;
}
int oband_seeded(int nnz, int nnx, const double *veln, const int64_t *velpn, const double *vel_map,
                 const int64_t *stif, const double *av_, const double *ph_, int ncol, double dnx, double dnz,
                 long nseed, const int32_t *seed_cell, const double *seed_t, double cdelta, double vmax, double r0,
                 double cdelta_far, double r_far, double *ttn, long *steps_out) {
    base_t bb;
    if (make_base(&bb, nnz, nnx, veln, velpn, vel_map, stif)) return -1;
    table_t tav = {av_, ncol}, tph = {ph_, ncol};
    loopcfg_t c = {&tav, &tph, dnx, dnz, 0, 0, 0, 0, 0, 0.0};
    memset(ttn, 0, sizeof(double) * (size_t)nnz * nnx);
    bstate_t b;
    if (bstate_alloc(&b, nnz, nnx, ttn)) return -1;
    fstate_t *f = &b.f;
    long nx = nnx, nz = nnz;
    for (long k = 0; k < nseed; k++) {
        long s = seed_cell[k];
        if (s < 0 || s >= nz * nx || f->nsts[s] == S_KNOWN) { bstate_free(&b, 0); free_base(&bb); return -2; }
        f->ttn[s] = seed_t[k];
        f->nsts[s] = S_KNOWN;
    }
    long nC = 0;
    for (long k = 0; k < nseed; k++) {
        long iz = seed_cell[k] / nx, ix = seed_cell[k] % nx;
        long nb[4][2] = {{iz, ix - 1}, {iz, ix + 1}, {iz - 1, ix}, {iz + 1, ix}};
        for (int q = 0; q < 4; q++) {
            long z = nb[q][0], x = nb[q][1];
            if (z < 0 || z >= nz || x < 0 || x >= nx) continue;
            long r = z * nx + x;
            if (f->nsts[r] == S_FAR) { f->nsts[r] = S_FARC; b.C[nC++] = (int32_t)r; }
        }
    }
    qsort(b.C, (size_t)nC, sizeof(int32_t), cmp_i32);
    for (long k = 0; k < nC; k++) {
        long r = b.C[k], iz = r / nx, ix = r % nx;
        double v = oref_update_f(f, &bb.m, c.ph, iz, ix, dnx, nz, nx);
        if (g_log.on) log_entry(r, -1, 1 | (v == -1.0 ? 2 : 0));
        if (v == -1.0) v = oref_fouds18_f(f, &bb.m, c.av, iz, ix, dnx, dnz, nx, nz);
        b.V[k] = v;
    }
    for (long k = 0; k < nC; k++) {
        long r = b.C[k];
        f->ttn[r] = b.V[k];
        f->nsts[r] = S_CLOSE;
        b.L[b.nL++] = (int32_t)r;
    }
    long steps = band_run(&b, &bb.m, &c, cdelta * dnx / vmax, 1, r0 * dnx / vmax, cdelta_far * dnx / vmax,
                          r_far > 0 && cdelta_far > 0 ? r_far * dnx / vmax : 0.0);
    bstate_free(&b, 0);
    free_base(&bb);
    if (steps_out) *steps_out = steps;
    return 0;
}

/* travel_finer_grid() as the device runs it (host_travel.cpp travel_chunk, sg > 1): the reference's two
 * heap stages (x9, x3) and the heap-ordered prefix of the fine main loop (fmm_exact.hip /
 * fmm_exact_lds.hip), then the band (fmm_band_k.hip mode 1) on the fine view, then / sg
 * (scale_kernel).  The stages and the hand-overs are travel_finer_impl()'s, unchanged.
 *
 * Where the device's rule decides:
 *  - tstop = (size2 + exact_r) dnx / vmax (host_travel.cpp travel_chunk: P.tstop) with the COARSE dnx; the walk stops
 *    before popping a root with key >= tstop (fmm_exact.hip:188), also at exact_r 0 (the device has
 *    no "prefix off": tstop is then the stage-2 window's radius).
 *  - the close list handed over is the heap (fmm_exact.hip:443-447; order is irrelevant to the band:
 *    acceptance and the Jacobi evaluation do not depend on it); the written box (bbox) only limits
 *    what the band kernel copies into its working field (fmm_band_k.hip:623-641) and has no
 *    arithmetic effect, so the model has no counterpart of it.  The LDS walk's window
 *    (fmm_exact_lds.hip:792-800) ends a walk that comes within 3 nodes of it with error 9, after
 *    which the HBM walk runs the source again: both give the prefix modelled here.
 *  - the band: delta = cdelta dnx / vmax, t0 = r0 dnx / vmax, the far band with
 *    delta_far = cdelta_far dnx / vmax past tfar = r_far dnx / vmax only when both are > 0
 *    (fmm_band_k.hip:675-678; host_travel.cpp travel_chunk passes cdelta_far 0 when sg > far_sg: the caller's rule),
 *    update() with the coarse dnx, fouds18_A() with the coarse dnx / dnz, on the quantised fine view.
 *  - the source must lie on the coarse grid (host_travel.cpp travel_chunk: the sg > 1 source check): -2 otherwise.
 * info[6]: band steps, nodes the prefix popped, close nodes handed over, peak heap entries of
 * stage 1, stage 2 and the prefix. */
int oband_travel_finer(double scx, double scz, int nz0, int nx0, const double *veln, const int64_t *velpn,
                       const double *vel_map, const int64_t *stif, const double *av_, const double *ph_, int ncol,
                       int sg_, double gox, double goz, double dnx, double dnz, double cdelta, double vmax,
                       double r0, double exact_r, double cdelta_far, double r_far, double *out, long *info) {
    long sg = sg_;
    if (sg < 1 || sg % 2 == 0) return -3;
    base_t bb;
    if (make_base(&bb, nz0, nx0, veln, velpn, vel_map, stif)) return -1;
    const mat_t *coarse = &bb.m;
    table_t tav = {av_, ncol}, tph = {ph_, ncol};
    const table_t *av = &tav, *ph = &tph;
    long csx = pyround((scx - gox) / dnx), csz = pyround((scz - goz) / dnz);
    if (csx < 0 || csx >= nx0 || csz < 0 || csz >= nz0) { free_base(&bb); return -2; }
    view_t vf;
    if (make_view(&vf, coarse, 0, coarse->nnz - 1, 0, coarse->nnx - 1, sg)) { free_base(&bb); return -1; }
    int64_t *zero_stif = NULL;
    if (coarse->stif == NULL) { /* stif_den0 is None -> zeros (:2159-2160) */
        zero_stif = (int64_t *)calloc((size_t)nz0 * nx0 * 5, sizeof(int64_t));
        vf.m.stif = zero_stif;
    }
    const mat_t *fine = &vf.m;
    long nnz = fine->nnz, nnx = fine->nnx;
    long isx = sg * csx, isz = sg * csz;
    int rc = 0;

    /* ---- stage 1: x9 ---- */
    long size1 = 2 * sg + (sg - 1) / 2, s1 = 9;
    long side1 = (s1 - 1) / 2 + s1 * ((sg - 1) / 2);
    long left = imax(0, isx - size1), right = imin(nnx - 1, isx + size1);
    long bottom = imax(0, isz - size1), top = imin(nnz - 1, isz + size1);
    view_t v1;
    fstate_t f1;
    if (make_view(&v1, fine, bottom, top, left, right, s1)) return -1;
    if (fstate_alloc(&f1, v1.m.nnz, v1.m.nnx, 0, NULL)) return -1;
    long isx_1 = s1 * (isx - left), isz_1 = s1 * (isz - bottom);
    double dnx1 = dnx / s1;
    straight_rays(&f1, isz_1, isx_1, side1, dnx1, fine, (int)isz, (int)isx, av, 1);
    add_edges(&f1, isz_1, isx_1, side1);
    loopcfg_t c1 = {av, ph, dnx1, dnx1, 1, (int)isx_1, (int)isz_1, (int)(s1 * size1), 0, 0.0};
    if (fmm_loop(&f1, &v1.m, &c1)) rc = -1;
    long peak1 = f1.peak;

    /* ---- stage 2: x3 ---- */
    long size2 = size1 + 3 * sg, s2 = 3;
    left = imax(0, isx - size2); right = imin(nnx - 1, isx + size2);
    bottom = imax(0, isz - size2); top = imin(nnz - 1, isz + size2);
    view_t v2;
    fstate_t f2;
    if (make_view(&v2, fine, bottom, top, left, right, s2)) return -1;
    if (fstate_alloc(&f2, v2.m.nnz, v2.m.nnx, 0, NULL)) return -1;
    long isx_2 = s2 * (isx - left), isz_2 = s2 * (isz - bottom);
    double dnx2 = dnx / s2;
    if (!rc && handover(&f1, isz_1, isx_1, &f2, isz_2, isx_2)) rc = -1;
    loopcfg_t c2 = {av, ph, dnx2, dnx2, 1, (int)isx_2, (int)isz_2, (int)(s2 * size2), 0, 0.0};
    if (!rc && fmm_loop(&f2, &v2.m, &c2)) rc = -1;
    long peak2 = f2.peak;
    fstate_free(&f1, 1);
    free_view(&v1);

    /* ---- fine grid: hand-over and the heap-ordered prefix ---- */
    size_t n = (size_t)nnz * nnx;
    fstate_t f;
    memset(out, 0, n * sizeof(double));
    if (fstate_alloc(&f, (int)nnz, (int)nnx, 0, out)) return -1;
    if (!rc && handover(&f2, isz_2, isx_2, &f, isz, isx)) rc = -1;
    fstate_free(&f2, 1);
    free_view(&v2);
    long known0 = 0, known1 = 0;
    for (size_t i = 0; i < n; i++) known0 += f.nsts[i] == 0;
    loopcfg_t c = {av, ph, dnx, dnz, 0, 0, 0, 0, 0, 0.0};
    loopcfg_t ce = c;
    ce.tstop = ((double)size2 + exact_r) * dnx / vmax;
    if (!rc && fmm_loop(&f, fine, &ce)) rc = -1;
    for (size_t i = 0; i < n; i++) known1 += f.nsts[i] == 0;

    /* ---- heap state -> band state (known, close = in the heap, far), then the band ---- */
    bstate_t bm;
    if (bstate_alloc(&bm, (int)nnz, (int)nnx, out)) return -1;
    for (size_t i = 0; i < n; i++) {
        if (f.nsts[i] == 0) bm.f.nsts[i] = S_KNOWN;
        else if (f.nsts[i] > 0) push_close(&bm, (long)i);
    }
    long nclose = bm.nL, peakp = f.peak;
    fstate_free(&f, 0);
    int far = r_far > 0 && cdelta_far > 0;
    long steps = 0;
    if (!rc)
        steps = band_run(&bm, fine, &c, cdelta * dnx / vmax, 1, r0 * dnx / vmax, cdelta_far * dnx / vmax,
                         far ? r_far * dnx / vmax : 0.0);
    bstate_free(&bm, 0);
    for (size_t i = 0; i < n; i++) out[i] = out[i] / (double)sg;
    free_view(&vf);
    free(zero_stif);
    free_base(&bb);
    if (info) {
        info[0] = steps; info[1] = known1 - known0; info[2] = nclose;
        info[3] = peak1; info[4] = peak2; info[5] = peakp;
    }
    return rc;
}
