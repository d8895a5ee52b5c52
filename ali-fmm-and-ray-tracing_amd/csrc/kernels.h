// kernels.h — parameter blocks and launchers shared by the kernels and the C-ABI host code.
#pragma once
#include "device_common.h"
#include "fmm_shared.h"
#include "solve_ops.h"  // the sums' geometry (kSolveMaxParts) of the resident sensitivity operator (sens_solve.hip)
#include "tfm_term.h"  // af::TfmParams: the parameter block of the TFM kernel (tfm.hip) and of its host model
#include "tfm_coh_term.h"  // af::TfmCohParams: the same of the coherence-weighted TFM kernel (tfm_coh.hip)
#include "tfm_model_term.h"  // af::TfmModelParams: the same of the FMC modelling kernel (tfm_model.hip)
#include "tfm_solve_ops.h"  // af::TfmLsqDims: the vectors' shapes of the least-squares imaging solve (tfm_solve.hip)
#include "tfm_sparse_ops.h"  // the scalars and partial arrays of sparsity-regularised imaging (tfm_sparse.hip)
#include "trace_fir_term.h"  // the trace FIR's sum and tile walk (trace_fir.hip)
#include "trace_fft_term.h"  // the spectral trace filter's arithmetic and passes (trace_fft.hip)
#include "trace_pick_term.h"  // the time-of-flight picker's rules (trace_pick.hip)

namespace af {

// per-source exchange block of the K-member band kernel (fmm_band_k.hip); zeroed by the host
// before each launch.  x1[member][step parity] = (step + 1) << 32 | payload words
// [Tmin lo, Tmin hi, live close cells, err << 24 | rim-list length], each written by its member
// with one sc1 store per step.
constexpr int kMaxK = 16;
struct KX {
  unsigned long long x1[kMaxK][2][4];
};

// one source of a band launch (fmm_exact_kernel / fmm_band_k_kernel); lists are split into K
// per-member slices (capL / K, capC / K) that spill the LDS lists of the band kernel
struct BandSrc {
  double* T;      // field (main grid, row-major): the result (fmm_band_k's copy-out writes it)
  double* Tb;     // the band kernel's working field (layout fmm_band_k.hip TbLayout), its two edge
                  // buffers after it
  int* S;         // status, row-major: fmm_exact_kernel's (mode 1), read by the band's hand-over
  int* Sb;        // the band kernel's status (layout fmm_band_k.hip SbLayout): far -1, known 0,
                  // close 1 + close-set slot
  int* Lin;       // mode 1: close cells handed over by fmm_exact_kernel (nl0 of them)
  int* L;         // close set: cells
  double* Lt;     // close set: T
  int* FS;        // free close-set slots
  int* A;         // accepted cells of the step
  int* C;         // claimed cells of the step
  int* Cp;        // their close-set slot (-1: far)
  double* V;      // claimed cells' new values
  int* Bl;        // claimed cells next to other members' columns
  int* Bp;        //   and their close-set slots
  int* D;         // edge cells accepted in the step (copied forward next step)
  double* Dv;     //   and their T
  int* Rx;        // claim items from other members' rim cells
  int* rimc;      // [K][2][capR] published close rim cells (packed cell)
  double* rimt;   //   and their T
  double* E;      // edge buffers [2][ecells] (4 columns per stripe, column-major: KGeom::eidx)
  KX* kx;
  double* Ts[2];  // stage grids (mode 1)
  int* Ss[2];
  int bbox[4];    // mode 1: rows / columns [z0, z1, x0, x1] of the main grid fmm_exact_kernel wrote
  long long steps[4];
  long long nupd;  // relax evaluations (cell-sweeps) in the main run
  long long t_begin, t_end;  // wall clock (100 MHz) when member 0 entered / left the band kernel
  int err;
  int nl0;
  // band profile (BandParams::prof): wall-clock ticks (100 MHz) of thread 0 of member 0 per phase
  // [Tmin + X1, accept + rim read, claim, evaluate, fallback, commit], list-size sums [close,
  // accepted, evaluated], max close, sub-phases [X1 wait, rim read, claim dedupe, drain before X1]
  long long ph[6];
  long long lsum[3];
  long long lmax;
  long long sub[4];
  int init_reused;  // mode 0: fmm_init_kernel left this source's hand-over as it was (InitSig); it
                    // writes this word when the chunk's own launch initialises the source
};

struct BandParams {
  DevModel M;
  int nsrc;
  int mode;      // 0: travel (subgrid 1, init from fmm_init_kernel); 1: travel_finer_grid
  int sg;        // subgrid size (mode 1)
  int nz, nx;    // main grid (fine grid in mode 1)
  double dnx, dnz;
  double cdelta, vmax, r0;
  double cdelta_far, r_far;  // band width beyond r_far nodes (0: off), ramped in over r_far .. 2 r_far
  double tstop;  // mode 1: the exact main-loop prefix stops when the heap root reaches it (fmm_exact_kernel)
  int exact_r;   // mode 1: tstop = (stage-2 half-width + exact_r) dnx / vmax (fmm_exact_lds: its window)
  int capL, capC, capS;  // list capacities, stage-grid capacity (cells)
  BandSrc* src;
  const HandoverOut* ho;  // mode 0
  const double* scx;
  const double* scz;
  double gox, goz;
  int prof;  // record BandSrc::ph / lsum (thread 0 reads the wall clock after each barrier)
  int coop;  // 1: hipLaunchCooperativeKernel (default); 0: plain launch after a residency check (under rocprofv3)
  int K;     // fmm_band_k: members per source (power of two <= kMaxK)
  int wlog;  // fmm_band_k: stripe width log2
  int xcd_local;  // fmm_band_k: 1 = plain cross-member stores once every member reports one XCD; 0 = always sc1
  int capR;  // fmm_band_k: rim-list capacity per member and parity
  long ecells;  // fmm_band_k: cells per edge buffer
  int tb_pitch;   // fmm_band_k: working-field pitch (bricks per brick row, or row pitch)
  long tb_cells;  // fmm_band_k: working-field size in doubles (the edge buffers follow)
  int sb_pitch;   // fmm_band_k: status-array pitch
  long max_steps;  // fmm_band_k: a band still running after this many steps stops with error 8
  // fmm_band_k, mode 0: stream final tiles to the host while the band runs (hs null: off).  A tile
  // is W (stripe width) columns x 2^tr_log rows of one member's stripe; it is final once all its
  // cells are known (a per-member LDS counter).  Member m = src * K + member owns rslots slots of
  // W << tr_log doubles in hs (coherent pinned host memory); its i-th final tile goes to slot
  // i mod rslots (row-major, row pitch W), then entry i = (i + 1) << 32 | tz * nstripes + stripe
  // to its host queue hq + m * qcap; the slot is reused once hcons[m] (host-written: tiles taken)
  // exceeds i
  double* hs;
  unsigned long long* hq;
  const unsigned* hcons;
  int qcap;
  int rslots;
  int tr_log;  // tile rows log2 (own tiles per member <= 1024, <= 32768 cells a tile)
};

struct RayJob {
  const double* ttf;  // receiver travel-time field on the fine grid (row-major, fnz x fnx)
  double sx, sy;      // source (fine-grid x, z)
  double rx, ry;      // receiver (fine-grid x, z)
};

struct RayParams {
  DevModel M;  // coarse model (veln f64, velpn, vel_map f64, stiffness)
  int fnz, fnx;
  int sg;
  double dnx;
  int nrays;
  int max_pts;
  const RayJob* jobs;
  double* ray_x;  // [nrays][max_pts]
  double* ray_y;
  int* ray_len;
  double* times;
  int* flags;     // bit0 early exit ("Travel time to receiver increasing"), bit1 capacity, bit2 empty plane
  int glanes;     // lanes per ray (af_ray_group_lanes)
};

struct LocalOpsParams {
  // 0 update() (update_ref), 1 fouds18_A(), 2 fouds18_A() as the band kernel runs it (resident model);
  // test entries for the forms the field kernels run: 3 update() on a register neighbourhood
  // (NbFieldT::load + update_nb), 4 the same selected over a wavefront (update_select_lanes),
  // 5 fouds18_A() on four lanes (fouds18_part<false>, f18_min, fouds18_combine), 6 the same with
  // fouds18_part<true> on the resident model
  int op;
  long n;
  int pz, px;
  const double* ttn;  // [n][pz][px]; ops 3, 4: NaN where nsts < 0 (the HBM grids' coding)
  const int* nsts;
  const int* iz;
  const int* ix;
  const double* dnx;
  const double* dnz;
  const int* nnz_arg;
  const int* nnx_arg;
  const double* cveln;  // material at the target cell, per case
  const int* cvelpn;
  const double* cvm;
  const double* cstif;  // [n][5] or nullptr (None)
  const double* tab;    // (361, ncol): phase table for update(), group table for fouds18_A()
  int ncol;
  double* out;
  // op 2: material of resident-model cell (mz, mx) under MatView::quant, through the per-material
  // record (band_mat<true>) and the precomputed slownesses DevModel::mslo (fouds18<true>)
  DevModel RM;
  const int* mz;
  const int* mx;
  int quant;
};

// alifmm_ray_sens (ray_sens.hip): rays ray0 .. ray0 + nrays - 1 of a request, whose packed points
// (x, z interleaved) lie in xy from the request's point pt0 on.  The per-ray arrays cover the whole
// request and are indexed by the ray's number in it.
struct SensParams {
  DevModel M;
  int sg;
  double dnx;
  int ray0, nrays;
  const double* xy;
  long long pt0;
  const long long* off;  // first point of each ray (prefix sum of the lengths)
  const int* len;        // points per ray
  const int* flags;      // nullable: rays with bit 1 or 2 are skipped
  const double* w;       // nullable: ray weights of the maps (1)
  long long* cnt;        // entries per ray: written by the count kernel (0 for a skipped or an invalid
                         // ray), read by the fill kernel
  int* status;           // count kernel: 1 for an invalid ray, else 0
  const long long* row;  // fill, rows: first entry of each ray
  int* col;              // fill, rows (each nullable)
  double* elen;
  double* etime;
  double* edth;
  double* maps;          // fill, nullable: [3][nz0][nx0], zeroed by the host
};

// alifmm_sens_op_* (sens_solve.hip): one quantity of the request's Jacobian, resident on the device.
// A[k][c] = cs[c] * sum of val[e] over the entries e of row k with col[e] == c; rows unmerged.
struct SensOp {
  int nrays;
  int nz, nx;
  long ncell;
  long long entries;         // < 2^31
  const long long* row_ptr;  // CSR [nrays + 1]: the fill pass's order (ray, then walk order)
  const int* col;
  const double* val;
  const long long* col_ptr;  // CSC [ncell + 1]: a column's entries in ascending entry index
  const int* row;
  const double* cval;
  const double* cs;          // [ncell] or null (1)
  const int* cols[3];        // the non-empty columns by length class (solve_ops.h: thread, wave, workgroup)
  int ncols[3];
};

// device vectors and scalars of alifmm_sens_op_solve
enum { kSolGamma = 0, kSolAlpha, kSolBeta, kSolReport, kSolBreak, kSolNorm, kSolScalars = 8 };
struct SolveVecs {
  double *x, *p, *s, *t, *xs;  // [ncell]; t = Aᵀ r, xs = cs p (the row product's scratch)
  double *r, *q;          // [nrays]
  double* parts;          // [kSolveMaxParts] partial sums
  double* scal;           // [kSolScalars]: gamma, alpha, beta, the iteration's report (the new gamma, or
                          // -1 when |q|² was 0), the breakdown flag, the last af_launch_solve_norm
  double damp2, smooth2;
};

// device vectors and scalars of alifmm_tfm_sparse (tfm_sparse.hip)
struct SparseVecs {
  double *x, *xn, *y, *g, *t;  // [nimg]: the iterate, the trial x⁺, the momentum point, the gradient at y, t = Bᵀ r
  double *d, *bx, *bxn, *r;    // [ndata]: the data, B x, B x⁺, r = B y - d
  double* parts;               // [kSpPartArrays][kSolveMaxParts] partial sums
  double* scal;                // [kSpScalars] (tfm_sparse_ops.h)
  double damp2, smooth2;
};

// the trace FIR (trace_fir.hip): out = P in (transpose 0) or Pᵀ in (1) over ntrace traces of nt
// samples; in and out distinct device vectors [ntrace][nt][ncomp], taps [ntap][tap_comp] on the device
struct TraceFirParams {
  const double* in;
  double* out;
  const double* taps;
  int64_t ntrace;
  int nt, ntap, origin, transpose;
};

// the spectral trace filter (trace_fft.hip): ntrace traces in [ntrace][S.nt][ncomp] -> out [ntrace][S.nt][2],
// distinct device arrays of float64 or float32; hrev the response on the device in element order,
// hrev[idx][S.resp_comp] = H[bitrev(idx)] (null: none)
struct TraceFftParams {
  const void* in;
  void* out;
  const double* hrev;
  int64_t ntrace;
  FftShape S;
};

// the time-of-flight picker (trace_pick.hip): ntrace traces in [ntrace][nt][ncomp] of float64 or float32
// and a gate [lo[t], hi[t]) per trace on the device -> six outputs per trace; mode 0 peak, 1 onset
// (0 < frac <= 1), guard >= 0
struct TracePickParams {
  const void* in;
  const int* lo;
  const int* hi;
  int64_t ntrace;
  int nt, mode, guard;
  double frac;
  double *pos, *amp, *amp2;
  int *idx, *idx2, *flags;
};

}  // namespace af

extern "C" {
// sig: a signature per slot of out (null: none); reuse: skip the walk of a slot whose signature matches;
// reused[i * reused_stride] (null: none): 1 when source i's walk was skipped, else 0
hipError_t af_launch_init(const af::DevModel* M, af::InitJob* jobs, int njobs, af::HandoverOut* out, af::InitSig* sig,
                          int reuse, int* reused, int reused_stride, hipStream_t stream);
hipError_t af_launch_exact(const af::BandParams* P, hipStream_t stream);
hipError_t af_launch_exact_lds(const af::BandParams* P, hipStream_t stream);
int af_exact_lds_fits(int sg, int exact_r);  // fmm_exact_lds holds the stage grids of subgrid sg
hipError_t af_launch_band_k(const af::BandParams* P, hipStream_t stream);
// the band kernel's working-field layout: pitch and size (doubles) for an nz x nx main grid
int af_band_tb_pitch(int nx);
long af_band_tb_cells(int nz, int nx);
int af_band_sb_pitch(int nx);
long af_band_sb_cells(int nz, int nx);
// working fields -> the row-major result fields of every source of the launch
hipError_t af_launch_scale(double* T, long n, double sg, hipStream_t stream);
hipError_t af_launch_rays(const af::RayParams* P, hipStream_t stream);
int af_ray_waves_per_simd();
int af_ray_group_lanes(int sg, int packed);
hipError_t af_launch_pack_rays(const double* rx, const double* ry, const int* len, const long long* off, int nrays,
                               int max_pts, double* packed, hipStream_t stream);
// back-wall echo paths (skip_pairs.hip).  Pick: W[f][q] = fld[f] at node (w_iz[q], w_ix[q]) for the nfld
// distinct fields of a request, then per pair the (value, node) minimum over W[row_a] + W[row_b].
// Join: legs 2 p and 2 p + 1 of the ray kernel's point buffers (leg_len [2 npairs]) -> pair p's joined
// ray at point off[p] of packed (replaces af_launch_pack_rays for such a launch)
hipError_t af_launch_skip_pick(const double* const* fld, int nfld, const int* w_iz, const int* w_ix, int fnx, int nw,
                               double* W, const int* row_a, const int* row_b, int npairs, double* pick_time, int* hit,
                               hipStream_t stream);
hipError_t af_launch_skip_join(const double* rx, const double* ry, const int* leg_len, const long long* off, int npairs,
                               int max_pts, double* packed, hipStream_t stream);
hipError_t af_launch_local_ops(const af::LocalOpsParams* P, hipStream_t stream);
// cr_math.h's functions on n arguments, one per thread (fn 0 atan, 1 sin, 2 cos, 3 tan -> out;
// 4 sincos -> out, out2): with the tables in global memory (utils.hip) and in LDS (cr_eval.hip)
hipError_t af_launch_cr_eval(int fn, long long n, const double* x, double* out, double* out2, hipStream_t stream);
hipError_t af_launch_cr_eval_lds(int fn, long long n, const double* x, double* out, double* out2, hipStream_t stream);
hipError_t af_launch_mat_slowness(const af::DevModel* M, double* out, hipStream_t stream);
hipError_t af_launch_tbp(const af::DevModel* M, int n, const double* x1, const double* x2, const double* y1,
                         const double* y2, double dnx, int sg, double* out, hipStream_t stream);
// TFM delay-and-sum (tfm.hip); chunk = receivers per register chunk: 4, 8, 16 or 32
hipError_t af_launch_tfm(const af::TfmParams* P, int chunk, hipStream_t stream);
// the same over the float64 samples P->fmc64
hipError_t af_launch_tfm_f64(const af::TfmParams* P, int chunk, hipStream_t stream);
// coherence-weighted TFM (tfm_coh.hip): the image, the factor of `kind` (1 CF, 2 SCF, 3 PCF: ncomp 2
// only) and, where Q->sums is set, its raw sums; chunk as in af_launch_tfm
hipError_t af_launch_tfm_coh(const af::TfmCohParams* Q, int kind, int chunk, hipStream_t stream);
// FMC modelling, the transpose of the TFM sum (tfm_model.hip); P->tile from af::tfm_model_tile(),
// P->slabs 1 .. 64 (> 1: P->out zeroed beforehand)
hipError_t af_launch_tfm_model(const af::TfmModelParams* P, hipStream_t stream);
// travel-time sensitivities along rays (ray_sens.hip): the count pass, then the fill pass
hipError_t af_launch_sens_count(const af::SensParams* P, hipStream_t stream);
hipError_t af_launch_sens_fill(const af::SensParams* P, hipStream_t stream);
// the resident sensitivity operator (sens_solve.hip).  Transpose: the CSC copy of a CSR (stable radix
// sort by column), key / key2 / idx / idx2 [entries] and temp (af_solve_sort_temp bytes) being scratch;
// classify: the non-empty columns by length class, counted (cols null) or listed from the cursors in
// cursor3 on; the products; CGLS: the start from t = Aᵀ rhs, one iteration, |v|² into scal[kSolNorm]
size_t af_solve_sort_temp(long long entries, long ncell);
hipError_t af_launch_solve_transpose(const af::SensOp* A, long long* col_ptr, int* row, double* cval, unsigned* key,
                                     unsigned* key2, unsigned* idx, unsigned* idx2, void* temp, size_t temp_bytes,
                                     hipStream_t stream);
hipError_t af_launch_solve_classify(const long long* col_ptr, long ncell, int* cols, int* cursor3, hipStream_t stream);
hipError_t af_launch_solve_rowprod(const af::SensOp* A, const double* x, double* xs, double* out, hipStream_t stream);
hipError_t af_launch_solve_colprod(const af::SensOp* A, const double* y, double* out, hipStream_t stream);
hipError_t af_launch_solve_start(const af::SensOp* A, const af::SolveVecs* V, hipStream_t stream);
hipError_t af_launch_solve_iter(const af::SensOp* A, const af::SolveVecs* V, hipStream_t stream);
hipError_t af_launch_solve_norm(const double* v, long n, const af::SolveVecs* V, hipStream_t stream);
// stage 2 of a two-stage sum over parts[nparts] and the scalar that follows from it: what 0 the norm,
// 1 alpha, 2 the new gamma and beta, 3 the start (sens_solve.hip solve_scalar_kernel)
hipError_t af_launch_solve_scalar(int what, const double* parts, int nparts, double* scal, hipStream_t stream);
// least-squares imaging (tfm_solve.hip): the dense window's pixel list for af_launch_tfm_model; after
// q = A p, alpha and x += alpha p, r -= alpha q; after t = Aᵀ r, s = t - R(x), gamma, beta (start:
// gamma_0, beta 0, p zeroed by the caller) and p = s + beta p.  V->xs is not used.
hipError_t af_launch_tfm_lsq_pix(int iz0, int ix0, int step, int fnx, int niz, int nix, int64_t* pix, hipStream_t stream);
hipError_t af_launch_tfm_lsq_step(const af::TfmLsqDims* G, const af::SolveVecs* V, hipStream_t stream);
hipError_t af_launch_tfm_lsq_grad(const af::TfmLsqDims* G, const af::SolveVecs* V, int start, hipStream_t stream);
// sparsity-regularised imaging (tfm_sparse.hip): the fused passes between the products of a FISTA
// iteration; each sums in two stages and leaves its scalars in V->scal (tfm_sparse_ops.h)
hipError_t af_launch_tfm_sparse_start(const af::TfmLsqDims* G, const af::SparseVecs* V, const double* rr, hipStream_t stream);
hipError_t af_launch_tfm_sparse_power_scale(const af::TfmLsqDims* G, const af::SparseVecs* V, hipStream_t stream);
hipError_t af_launch_tfm_sparse_power(const af::TfmLsqDims* G, const af::SparseVecs* V, hipStream_t stream);
hipError_t af_launch_tfm_sparse_grad(const af::TfmLsqDims* G, const af::SparseVecs* V, hipStream_t stream);
hipError_t af_launch_tfm_sparse_prox(const af::TfmLsqDims* G, const af::SparseVecs* V, double step, double tau,
                                     hipStream_t stream);
hipError_t af_launch_tfm_sparse_trial(const af::TfmLsqDims* G, const af::SparseVecs* V, double L, hipStream_t stream);
hipError_t af_launch_tfm_sparse_momentum(const af::TfmLsqDims* G, const af::SparseVecs* V, double beta, hipStream_t stream);
hipError_t af_launch_tfm_sparse_final(const af::TfmLsqDims* G, const af::SparseVecs* V, hipStream_t stream);
// the trace FIR and its transpose (trace_fir.hip; the sum: trace_fir_term.h); ncomp 1 or 2, tap_comp 1 or
// 2 (2: ncomp 2), 1 <= ntap <= af::kFirMaxTaps, 0 <= origin < ntap.  af_trace_fir_tile: outputs per workgroup
hipError_t af_launch_trace_fir(const af::TraceFirParams* P, int ncomp, int tap_comp, hipStream_t stream);
int af_trace_fir_tile();
// the spectral trace filter (trace_fft.hip; the arithmetic: trace_fft_term.h); ncomp 1 or 2, dtype 0 float64 or
// 1 float32 (of in and out).  af_trace_fft_grid: the most workgroups a launch starts
hipError_t af_launch_trace_fft(const af::TraceFftParams* P, int ncomp, int dtype, hipStream_t stream);
int af_trace_fft_grid();
// the time-of-flight picker (trace_pick.hip; the rules: trace_pick_term.h); ncomp 1 or 2, dtype 0 float64 or
// 1 float32.  af_trace_pick_grid: the most workgroups a launch starts
hipError_t af_launch_trace_pick(const af::TracePickParams* P, int ncomp, int dtype, hipStream_t stream);
int af_trace_pick_grid();
}
