// context.h — the host-side context behind include/alifmm.h (one GPU): resident model, work
// arena, resident fields, the grow-only device buffers of every entry family (DevBuf), pinned
// staging ring.  Shared by the host units (host_*.cpp, through host_internal.h) and comm.cpp
// (RCCL gather of resident fields).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/alifmm.h"
#include "kernels.h"

template <class T>
static inline hipError_t dalloc(T** p, size_t n) {
  return hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T));
}
static inline void dfree(void* p) {
  if (p) (void)hipFree(p);
}
// Owning device buffer of n elements (capacity, not bytes), grown on demand and never shrunk.
// grow(need): nothing when the capacity suffices; otherwise the old buffer is freed first, then the
// new one allocated (the peak is one buffer, not two), at least one element; after a failed
// allocation the buffer is empty (capacity 0).  Move-only: a buffer is freed once, by release(),
// by an assignment (`group = {}` releases every buffer of a struct of them) or with its owner.
// Converts to its pointer, so launches and copies take it as they took the plain pointer.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, n = o.n;
      o.p = nullptr, o.n = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t grow(size_t need) {
    if (p && n >= need) return hipSuccess;
    release();
    const hipError_t e = dalloc(&p, need);
    if (e == hipSuccess) n = need;
    return e;
  }
  void release() {
    dfree(p);
    p = nullptr;
    n = 0;
  }
  operator T*() const { return p; }
};

struct Field {
  DevBuf<double> d;  // the field + the K-member band kernel's edge buffers after it
  size_t bytes = 0;  // the field (fnz x fnx doubles)
  int sg = 0, nz = 0, nx = 0;
  int64_t steps[4] = {0, 0, 0, 0};
  int64_t sweeps = 0;
  int64_t prof[14] = {};
  int64_t span[2] = {0, 0};  // band kernel: member 0's entry / exit wall clock (100 MHz ticks)  // band profile: 6 phase ticks, 3 list sums, max close, 4 sub-phase ticks
};

struct Arena {  // per-chunk scratch, reused across calls
  int nsrc = 0;
  long cells = 0, scells = 0, capL = 0, capC = 0, capS = 0;
  DevBuf<int> S;          // row-major status, scells per source (subgrid > 1 only)
  DevBuf<int> lists;      // Lin | FS | A | L | C | Cp | D | Rx | Bl | Bp per source
  DevBuf<double> dlists;  // Lt | V | Dv per source
  int K = 0;              // K-member kernel: members the rim lists are sized for
  long capR = 0, ecells = 0;
  DevBuf<int> rimc;       // K-member kernel: rim lists [src][K][2][capR]
  DevBuf<double> rimt;
  DevBuf<af::KX> kx;      // K-member kernel: exchange blocks
  DevBuf<double> Tb;      // band kernel: working fields + their edge buffers, tbc doubles per source
  long tbc = 0;
  DevBuf<int> Sb;         // band kernel: status arrays, sbc per source
  long sbc = 0;
  DevBuf<double> Ts;      // stage grids (travel_finer_grid), 2 per source
  DevBuf<int> Ss;
  DevBuf<af::BandSrc> srcs;
  // the source-init hand-overs, a signature per slot (allocated and zeroed with it) and the jobs,
  // sized together (host_travel.cpp ensure_handover): grown by a source-init launch alone, they
  // outlive every regrowth of the rest (ensure_arena)
  DevBuf<af::HandoverOut> ho;
  DevBuf<af::InitSig> sig;
  DevBuf<af::InitJob> jobs;
  DevBuf<double> dscx, dscz;
};


struct alifmm_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t fill = nullptr;  // field initialisation, overlapped with the source-init kernel
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // [4]: after the wait for the fill stream
  hipEvent_t ev_fill = nullptr;
  std::string err;
  // model
  bool have_model = false;
  int nz0 = 0, nx0 = 0, ncol = 0;
  double dnx = 0, dnz = 0, gox = 0, goz = 0, vmax = 0;
  struct ModelBufs {  // the resident model (DevModel points into these), released by set_model
    DevBuf<double> veln, vm;
    DevBuf<int> velpn, sidx;
    DevBuf<double> stab;
    DevBuf<int> mid;
    DevBuf<unsigned char> mid8;   // the same ids as bytes when there are <= 256 materials
    DevBuf<unsigned char> mid8b;  // ... in 8 x 16 bricks (DevModel::mid8b)
    DevBuf<af::MatRec> mtab;
    DevBuf<double> mslo;  // fouds18_A() slownesses per material (DevModel::mslo)
    DevBuf<double> gtab, ptab;
  } dm;
  int nstab = 0;
  int mid8b_pitch = 0;
  int nmat = 0;
  // options
  // band width (units of dnx / vmax): the caller's "cdelta" when set, else chosen from the model
  // (band_cdelta: 0.5, narrowed to 0.2 on models whose material changes from cell to cell)
  double cdelta = 0.5, r0 = 40.0;
  bool cdelta_set = false;
  double mat_jump = 0.0;  // set_model: fraction of 4-neighbour cell pairs whose materials differ
  // band width beyond r_far = 768 nodes (ramped in over 768 .. 1536): < 0 = 1.4 x the band width
  // in force (0.7 at 0.5); 0 = off; > 0 = the caller's, never narrower than the band width in force
  // (band_cdelta_far).  Round 6 sweep (profiles/r6_far_band_gpu_sweep.jsonl, GPU fields and rays
  // vs the reference's): C4 band 325 -> 311 ms at 128 sources, 148 -> 137 ms at 16, and every
  // error lower than round 5's 0.6 from 256 (F7 rays max 1.7e-3 -> 4.5e-4, C4 source field max
  // 1.0e-3 -> 5.3e-4, C3 7.4e-4 -> 6.5e-4; mean errors 1.1-2.2e-5 -> 1.4-1.9e-5)
  double cdelta_far = -1.0, r_far = 768.0;
  int far_sg = 1;  // largest subgrid the far band applies to (subgrid 9 weld rays: profiles/r5j)
  int exact_r = 20;
  void* team = nullptr;  // host_fields.cpp CopyTeam: host copy threads of the pinned staging ring
  int exact_lds = 1;  // subgrid > 1: the LDS exact walk (fmm_exact_lds.hip) when it fits (0: fmm_exact.hip)
  int batch = 256;
  // subgrid-1 source init of a whole multi-launch travel call (one init launch for every chunk)
  struct InitAllBufs {
    DevBuf<af::HandoverOut> ho;
    DevBuf<af::InitJob> jobs;
    DevBuf<af::InitSig> sig;  // a signature per slot of ho, allocated and zeroed with it
    DevBuf<int> reused;       // per source of that launch: its walk was skipped
  } all;
  // reuse of source-init hand-overs (fmm_shared.h InitSig): "init_reuse", "init_reused" (sources of
  // the last travel call whose walk was skipped)
  int init_reuse = 1;
  int init_reused = 0;
  // host copy of the small tables the walk reads (group and phase tables, the unique stiffness
  // rows in their order): set_model bumps tab_epoch when they differ byte for byte from the last
  // model's, so a signature of another epoch never matches
  unsigned tab_epoch = 0;
  int h_ncol = 0;
  std::vector<double> h_gtab, h_ptab, h_stab;
  const af::HandoverOut* ho_last = nullptr;  // what alifmm_init_profile reads (last travel call)
  int n_ho_last = 0;
  // alifmm_travel_seeded: the seeded hand-overs (a buffer of their own: the InitSig signatures vouch
  // for the arena's and all.ho only) and the call's geometry and times, grow-only, freed with the context
  struct SeedBufs {
    DevBuf<af::HandoverOut> ho;
    DevBuf<int> cell;            // seed cells, list order
    DevBuf<int> close;           // close cells, ascending
    DevBuf<int> win;             // [close][25] seed indices
    DevBuf<double> t;            // [nfield][nseed] host times
    DevBuf<const double*> from;  // [nfield] source fields
  } seed;
  double t_seed = 0;                   // last alifmm_travel_seeded: the seed pass (ms)
  long seed_nodes = 0, seed_close = 0; // its seeds and close cells
  int prof = 0;
  int coop = 1;  // band kernel: cooperative launch (1; 0 under rocprofv3) or plain launch after a residency check (0)
  int members = 0;     // band kernel: workgroups per source (0: as many as the device fits, <= 16)
  int stripe_log = 0;  // band kernel: stripe width log2 (0: 6 for K <= 4, 4 for K >= 8)
  int last_k = 0;      // members per source of the last band launch
  int xcd_local = 1;   // band kernel: plain cross-member stores once a source's members share an XCD (0: always sc1)
  int n_cu = 0;
  long cap_scale = 1;
  // state
  std::vector<Field> fields;
  Arena arena;
  double t_init = 0, t_band = 0, t_total = 0;
  double t_fill_wait = 0;  // last travel: ms the band launches waited for the fill stream after the source init ("fill_wait_ms")
  double t_ray_kernel = 0, t_ray_pack = 0, t_find_rays = 0, t_take_rays = 0;  // last find_rays / take_rays (ms)
  int last_ray_lanes = 0;  // lanes per ray of the last find_rays launch (rays.hip af_ray_group_lanes)
  // packed points of the last alifmm_find_rays(ray_xy = NULL, ray_xy_cap = ALIFMM_KEEP_RAYS) call,
  // per ray in the caller's order, until alifmm_take_rays() copies them out
  std::vector<std::vector<double>> kept_rays;  // host-staged (several subgrids in one call)
  struct KeptChunk {
    double* d;  // packed (x, z) points of a chunk of rays, device memory
    int64_t npts;
  };
  std::vector<KeptChunk> kept_dev;  // device-resident (one subgrid: the caller's order)
  int64_t kept_pts = 0;
  // ray-tracer work buffers, kept across alifmm_find_rays calls (sized for the largest chunk seen:
  // rx / ry hold its points, the others are per ray)
  struct RayBufs {
    DevBuf<double> rx, ry, t;
    DevBuf<int> len, flags;
    DevBuf<af::RayJob> jobs;
    DevBuf<long long> off;
  } rb;
  // alifmm_skip_pick / alifmm_skip_rays: grow-only device buffers (the distinct fields' pointer table,
  // the reflector nodes, W[field][node], the pairs' rows of W, the picks), freed with the context
  struct SkipBufs {
    DevBuf<const double*> tab;
    DevBuf<int> wiz, wix, row, hit;  // row: [2][npairs]
    DevBuf<double> W, pick;
  } skip;
  double t_skip_pick = 0, t_skip_join = 0;  // last skip_pick / skip_rays: the pick's kernels, the join kernel (ms)
  // pinned staging ring of alifmm_copy_fields (pageable destinations)
  static constexpr int kPinBufs = 4;
  static constexpr size_t kPinBytes = 32u << 20;
  void* pin[kPinBufs] = {};
  hipEvent_t pin_ev[kPinBufs] = {};
  // alifmm_travel_into (subgrid 1): the band kernel streams final tiles into a ring of slots per
  // band member (hstage: coherent pinned memory) and their indices into hq (per-member queues);
  // the copy team moves each tile on to the caller's field and returns its slot (hcons).  Kept
  // across calls (freed by alifmm_release_fields / alifmm_ctx_destroy).
  int stream_out = 1;
  void* hstage = nullptr;
  size_t hstage_bytes = 0;
  unsigned long long* hq = nullptr;
  size_t hq_bytes = 0;
  unsigned* hcons = nullptr;
  size_t hcons_bytes = 0;
  double t_stream_tail = 0;  // last travel_into: ms from the band kernel's end to the last tile copied
  long stream_fallback = 0;  // last travel_into: fields copied after the kernel (not streamed)
  long exact_redo = 0;       // last travel (subgrid > 1): sources the LDS exact walk handed to the HBM walk
  // alifmm_tfm: grow-only device buffers (data, pair weights, slot pointer table, image), freed
  // with the context
  struct TfmBufs {
    DevBuf<float> fmc;
    DevBuf<double> fmc64;  // alifmm_tfm_f64's data
    DevBuf<float> w;
    DevBuf<const double*> tab;
    DevBuf<double> img;
    DevBuf<double> coh_f, coh_s;  // alifmm_tfm_coh's factor and raw sums
  } tfm;
  int tfm_chunk = af::kTfmChunk;  // receivers per register chunk of the TFM kernel (4, 8, 16, 32)
  double t_tfm_upload = 0, t_tfm_kernel = 0;  // last alifmm_tfm (ms)
  double t_tfm_coh_upload = 0, t_tfm_coh_kernel = 0;  // last alifmm_tfm_coh (ms)
  // alifmm_tfm_model: grow-only device buffers (the non-zero pixels' field offsets and
  // reflectivities, pair weights, slot pointer table, modelled data), freed with the context
  struct TfmModelBufs {
    DevBuf<int64_t> pix;
    DevBuf<double> refl;
    DevBuf<float> w;
    DevBuf<const double*> tab;
    DevBuf<double> out;
  } tfm_model;
  int tfm_model_tile = 0, tfm_model_slabs = 0;            // the settings (0: automatic)
  int tfm_model_rx = af::kTfmModelRx;                     // receivers per workgroup (1, 2, 4)
  int tfm_model_combine = 12;  // a wave of at most this many runs of lanes sharing a sample sums each run before it adds
  int tfm_model_tile_used = 0, tfm_model_slabs_used = 0;  // what the last alifmm_tfm_model ran with
  double t_tfm_model_upload = 0, t_tfm_model_kernel = 0;  // last alifmm_tfm_model (ms)
  // alifmm_tfm_lsq: grow-only device buffers (r and q: 2 x the data, and w with a pulse: 3 x; x, p, s
  // and t: 4 x the image; the window's pixel list, pair weights, slot pointer table, partial sums +
  // scalars), freed with the context, or by a call whose allocation fails
  struct TfmLsqBufs {
    DevBuf<double> data, img, small;
    DevBuf<int64_t> pix;
    DevBuf<float> w;
    DevBuf<const double*> tab;
  } tfm_lsq;
  double t_tfm_lsq_upload = 0, t_tfm_lsq_kernel = 0;  // last alifmm_tfm_lsq / alifmm_tfm_lsq_pulse (ms)
  int tfm_lsq_iters = 0;
  // alifmm_tfm_sparse: grow-only device buffers (d, B x, B x⁺ and r: 4 x the data, and w with a pulse:
  // 5 x; x, x⁺, y, g and t: 5 x the image; the window's pixel list, pair weights, slot pointer table,
  // partial sums + scalars), freed with the context, or by a call whose allocation fails
  TfmLsqBufs tfm_sparse;
  double t_tfm_sparse_upload = 0, t_tfm_sparse_kernel = 0;  // last alifmm_tfm_sparse (ms)
  int tfm_sparse_iters = 0, tfm_sparse_backtracks = 0;
  double tfm_sparse_l0 = 0;  // the L its first iteration began with (given, or the power estimate)
  // alifmm_trace_fir: grow-only device buffers (the traces in and out, the taps; the taps also serve
  // alifmm_tfm_lsq_pulse), freed with the context
  struct FirBufs {
    DevBuf<double> in, out, taps;
  } fir;
  double t_fir_upload = 0, t_fir_kernel = 0;  // last alifmm_trace_fir (ms)
  // alifmm_trace_spectral: grow-only device buffers (the traces in and out, sized in doubles whatever
  // the dtype; the response in element order), freed with the context
  struct FftBufs {
    DevBuf<double> in, out, resp;
  } fft;
  double t_fft_upload = 0, t_fft_kernel = 0, t_fft_download = 0;  // last alifmm_trace_spectral (ms)
  // alifmm_trace_pick: grow-only device buffers (the gates lo then hi; pos, amp, amp2; idx, idx2,
  // flags), freed with the context.  Its traces live in fft.in and, filtered, in fft.out
  struct PickBufs {
    DevBuf<int> gates, outi;
    DevBuf<double> outd;
  } pick;
  double t_pick_upload = 0, t_pick_filter = 0, t_pick_kernel = 0, t_pick_download = 0;  // last alifmm_trace_pick (ms)
  // alifmm_ray_sens: grow-only device buffers (a chunk of host points, the per-ray arrays of a
  // request, the three maps), freed with the context; the row arrays live for one call
  struct SensBufs {
    DevBuf<double> xy;
    DevBuf<long long> off, cnt, row;
    DevBuf<int> len, flags, status;
    DevBuf<double> w, maps;
  } sens;
  double t_sens_upload = 0, t_sens_kernel = 0;  // last alifmm_ray_sens (ms)
  int64_t sens_entries = 0;                     // its entries (row_ptr[nrays])
  // alifmm_sens_op_*: the resident operator (CSR, CSC, column scale, column lists; A points into
  // these), freed by alifmm_sens_op_release, alifmm_set_model and with the context; and the grow-only
  // vectors of apply and solve, freed with the context
  struct SensOpBufs {
    bool have = false;
    af::SensOp A = {};
    DevBuf<long long> row_ptr, col_ptr;
    DevBuf<int> col, row, cols;
    DevBuf<double> val, cval, cs;
  } op;
  struct SolveBufs {
    DevBuf<double> cell, ray, small;  // 5 x ncell, 2 x nrays, partial sums + scalars
  } solve;
  double t_solve_build = 0, t_solve_kernel = 0;  // last sens_op_build (whole call) / apply or solve (device), ms
  int solve_iters = 0;                           // last alifmm_sens_op_solve
};

// the band width in force for the resident model on the subgrid-sg grid, and the far band's (0: off)
static inline double band_cdelta(const alifmm_ctx* c, int sg = 1) {
  if (c->cdelta_set) return c->cdelta;
  // CPU band model vs the heap oracle (tools/cdelta_auto_sweep.py, profiles/r6_cdelta_auto_sweep.jsonl):
  // at 0.5 every swept model stays below 6.1e-3 except per-cell random orientation + vel_map
  // (jump fraction ~1: 1.16e-2 on the 61^2 test model); at 0.2 every swept model is <= 4e-5.
  // The fraction is per pair of the band's grid (the model's / sg on the subgrid-sg grid); every
  // BASELINE config keeps 0.5 (C2 weld 0.178, C3 0.0066, C4 0.020)
  const double j = c->mat_jump / sg, j0 = 0.3, j1 = 0.6, lo = 0.2;
  if (j <= j0) return c->cdelta;
  if (j >= j1) return lo;
  return c->cdelta + (lo - c->cdelta) * (j - j0) / (j1 - j0);
}
static inline double band_cdelta_far(const alifmm_ctx* c, int sg = 1) {
  if (c->cdelta_far == 0.0) return 0.0;
  const double cd = band_cdelta(c, sg);
  return c->cdelta_far < 0 ? 1.4 * cd : std::max(c->cdelta_far, cd);
}

static inline int fail(alifmm_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HIPCHK(call)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) return fail(ctx, ALIFMM_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)


// slot `slot` holds an (fz, fx) field of subgrid sg (+ extra_cells doubles after it); host_travel.cpp
extern "C" int af_ensure_field(alifmm_ctx* ctx, int slot, int sg, int fz, int fx, long extra_cells = 0);
