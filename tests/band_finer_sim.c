/* The CPU band model of travel_finer_grid (oracle/band_model.c oband_travel_finer) run stand-alone
 * under ASan and UBSan (tests/test_band_finer_sim.py compiles this file together with
 * oracle/band_model.c): 2 x 2 at subgrid 9 (every stage window clipped on four sides), 12 x 9 with
 * a corner source at subgrid 3, 4 x 5 at subgrid 11 (the whole field inside the heap-ordered
 * prefix).  A model with table and Christoffel cells side by side, fractional orientations and a
 * vel_map that float32 does not hold.  Every field finite, zero at the source and positive
 * elsewhere; the reported counts consistent.  Prints "ok <fields>". */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int oband_travel_finer(double scx, double scz, int nz0, int nx0, const double *veln, const int64_t *velpn,
                       const double *vel_map, const int64_t *stif, const double *av_, const double *ph_, int ncol,
                       int sg_, double gox, double goz, double dnx, double dnz, double cdelta, double vmax,
                       double r0, double exact_r, double cdelta_far, double r_far, double *out, long *info);
double oref_group_vel(double angle, long c22, long c23, long c33, long c44, long sigma, double vel_scale);

static const int64_t kStif[5] = {249000, 133000, 205000, 125000, 7850};

static unsigned long long g_seed = 12345;
static double urand(void) {
    g_seed = g_seed * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(g_seed >> 11) / 9007199254740992.0;
}

static int run(int nz, int nx, int sg, int sx, int sz, int with_stif, double cdelta_far, double r_far) {
    size_t n = (size_t)nz * nx;
    double *veln = malloc(n * 8), *vm = malloc(n * 8), *tab = malloc(361 * 2 * 8);
    int64_t *velpn = malloc(n * 8), *stif = with_stif ? malloc(n * 5 * 8) : NULL;
    long fz = (long)sg * (nz - 1) + 1, fx = (long)sg * (nx - 1) + 1;
    double *out = malloc((size_t)fz * fx * 8);
    if (!veln || !vm || !tab || !velpn || (with_stif && !stif) || !out) return 1;
    for (int a = 0; a < 361; a++) { tab[2 * a] = a; tab[2 * a + 1] = 1.0; }
    double vchr = 0.0;
    for (int a = 0; a <= 3600; a++) vchr = fmax(vchr, oref_group_vel(0.05 * a, kStif[0], kStif[1], kStif[2], kStif[3], kStif[4], 1.0));
    double vmax = 0.0;
    for (size_t i = 0; i < n; i++) {
        veln[i] = 180.0 * urand();
        velpn[i] = with_stif ? (urand() < 0.3) : 1;
        vm[i] = velpn[i] ? 5790.0 : 1.0 + 0.2 * urand();
        vmax = fmax(vmax, velpn[i] ? vm[i] : vchr * vm[i]);
        if (with_stif) for (int k = 0; k < 5; k++) stif[5 * i + k] = kStif[k];
    }
    long info[6];
    const double dnx = 1e-3, dnz = 1e-3;
    int rc = oband_travel_finer(sx * dnx, sz * dnz, nz, nx, veln, velpn, vm, stif, tab, tab, 2, sg, 0.0, 0.0, dnx, dnz,
                                0.5, vmax, 40.0, 20.0, cdelta_far, r_far, out, info);
    int bad = rc != 0;
    for (long i = 0; i < fz * fx && !bad; i++) {
        int at_src = i == (long)sz * sg * fx + (long)sx * sg;
        if (!isfinite(out[i]) || (at_src ? out[i] != 0.0 : !(out[i] > 0.0))) bad = 2;
    }
    if (!bad && (info[0] < 0 || info[1] <= 0 || info[2] < 0 || info[2] > fz * fx || info[3] <= 0 || info[4] <= 0 ||
                 info[5] <= 0 || info[1] > fz * fx))
        bad = 3;
    if (bad) fprintf(stderr, "%d x %d sg %d source (%d, %d): rc %d bad %d\n", nz, nx, sg, sx, sz, rc, bad);
    /* an even subgrid and a source off the grid are refused, nothing is written past the arrays */
    if (!bad && oband_travel_finer(sx * dnx, sz * dnz, nz, nx, veln, velpn, vm, stif, tab, tab, 2, 4, 0.0, 0.0, dnx, dnz,
                                   0.5, vmax, 40.0, 20.0, 0.0, 0.0, out, info) != -3)
        bad = 4;
    if (!bad && oband_travel_finer((nx + 1) * dnx, 0.0, nz, nx, veln, velpn, vm, stif, tab, tab, 2, sg, 0.0, 0.0, dnx,
                                   dnz, 0.5, vmax, 40.0, 20.0, 0.0, 0.0, out, info) != -2)
        bad = 5;
    free(veln); free(vm); free(tab); free(velpn); free(stif); free(out);
    return bad;
}

int main(void) {
    int fields = 0;
    for (int sx = 0; sx < 2; sx++)
        for (int sz = 0; sz < 2; sz++, fields++)
            if (run(2, 2, 9, sx, sz, 1, 0.0, 0.0)) return 1;
    if (run(12, 9, 3, 0, 0, 1, 0.0, 0.0)) return 1;
    if (run(12, 9, 3, 8, 11, 1, 0.7, 8.0)) return 1; /* the far band engaged */
    if (run(12, 9, 3, 8, 0, 0, 0.0, 0.0)) return 1;  /* no stiffness: the zero rows */
    if (run(4, 5, 11, 2, 1, 1, 0.0, 0.0)) return 1;
    if (run(4, 5, 11, 4, 3, 1, 0.0, 0.0)) return 1;
    fields += 5;
    printf("ok %d\n", fields);
    return 0;
}
