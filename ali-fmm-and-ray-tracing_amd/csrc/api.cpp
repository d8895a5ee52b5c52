// api.cpp — host runtime behind include/alifmm.h (HIP, one context per GPU).
//
// Owns the HBM-resident model, the per-source work arena (status grid + band work lists) and
// the resident travel-time fields that the ray tracer reads without a host round trip.
// Sources are processed in launches of at most `batch` (and at most half the CUs: >= 2 band
// workgroups per source), all workgroups of a launch co-resident.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/alifmm.h"
#include "context.h"
#include "kernels.h"
#include "tile_stream.h"

extern char** environ;

static void free_ray_bufs(alifmm_ctx* c) {
  auto& b = c->rb;
  for (void* p : {(void*)b.rx, (void*)b.ry, (void*)b.t, (void*)b.len, (void*)b.flags, (void*)b.jobs, (void*)b.off})
    if (p) (void)hipFree(p);
  b = alifmm_ctx::RayBufs();
}
static void free_tfm_lsq_bufs(alifmm_ctx* c) {
  auto& b = c->tfm_lsq;
  dfree(b.data); dfree(b.img); dfree(b.small); dfree(b.pix); dfree(b.w); dfree(b.tab);
  b = alifmm_ctx::TfmLsqBufs();
}
// points kept by alifmm_find_rays(..., ALIFMM_KEEP_RAYS) for alifmm_take_rays
static void release_kept_rays(alifmm_ctx* c) {
  for (auto& k : c->kept_dev) dfree(k.d);
  c->kept_dev.clear();
  std::vector<std::vector<double>>().swap(c->kept_rays);
  c->kept_pts = 0;
}
static void free_arena(Arena& a) {
  dfree(a.S); dfree(a.lists); dfree(a.dlists); dfree(a.Ts); dfree(a.Ss); dfree(a.srcs); dfree(a.ho); dfree(a.sig); dfree(a.jobs);
  dfree(a.rimc); dfree(a.rimt); dfree(a.kx); dfree(a.Tb); dfree(a.Sb);
  dfree(a.dscx); dfree(a.dscz);
  a = Arena();
}

// ---- host-side velocity maximum (for the band width) ----
static double pymod(double a, double b) {
  double m = std::fmod(a, b);
  if (m != 0.0) {
    if ((b < 0) != (m < 0)) m += b;
  } else {
    m = std::copysign(0.0, b);
  }
  return m;
}
static double christoffel_group_host(const double* s, double eff, double vm) {
  double e90 = pymod(eff, 90);
  if (e90 < 0.01 || e90 > 90 - 0.01) {
    double lam = (std::fabs(pymod(eff, 180) - 90) < 1) ? s[2] : s[0];
    return 1000 * vm * std::sqrt(lam / s[4]);
  }
  double tan_ang = std::tan(eff * M_PI / 180.0);
  double A = s[0] + s[2] - 2 * s[3], B = (s[1] + s[3]) * (tan_ang - 1 / tan_ang), C = s[0] - s[2];
  double disc = B * B + A * A - C * C;
  double pa = eff < 90 ? pymod(std::atan((-B - std::sqrt(disc)) / (C - A)), M_PI)
                       : pymod(std::atan((-B + std::sqrt(disc)) / (C - A)), M_PI);
  double lam = 0.5 * (std::cos(2 * pa) * (s[0] - s[3]) + std::sin(2 * pa) * (s[1] + s[3]) * tan_ang + s[0] + s[3]);
  return 1000 * vm * std::sqrt(lam / s[4]) / std::cos(eff * M_PI / 180.0 - pa);
}

// material-id table capacity (the band kernel stages <= kMatLds of them in LDS)
static const int kMaxMatIds = 4096;
// plane-search candidates per ray the ray kernel holds (rays.hip kMaxCand)
static const int kMaxRayCand = 256;
// ray point buffers larger than this are freed at the end of each alifmm_find_rays call
static const size_t kRayBufKeepBytes = (size_t)1 << 30;

// host copies up to this size go straight to pageable memory while the pinned ring is unallocated
static const size_t kSmallD2H = (size_t)64 << 20;
// contexts alive in this process (copy teams share the process's CPU share between them)
static std::atomic<int> g_live_ctx{0};

// ---- set_model's per-cell passes over the host threads ----
// the process's CPU share (OMP_NUM_THREADS on the GPU box, else the hardware's, at most 32)
static int host_threads() {
  int n = (int)std::max(1u, std::thread::hardware_concurrency());
  if (const char* e = getenv("OMP_NUM_THREADS")) {
    const int v = atoi(e);
    if (v >= 1) n = v;
  }
  // contexts that upload models at the same time (update_parallel: one per GPU) share the share
  return std::max(1, std::min(n, 32) / std::max(1, g_live_ctx.load()));
}
// fn(chunk, lo, hi) over nch contiguous chunks of [0, n), one thread each
// (serially below min_n items: the default suits per-cell passes; row passes give a smaller one)
static void for_chunks(size_t n, int nch, const std::function<void(int, size_t, size_t)>& fn,
                       size_t min_n = 65536) {
  if (nch <= 1 || n < min_n) {
    fn(0, 0, n);
    return;
  }
  std::vector<std::thread> th;
  for (int c = 0; c < nch; c++) th.emplace_back(fn, c, n * c / nch, n * (c + 1) / nch);
  for (auto& t : th) t.join();
}
// Distinct keys of cells [0, n) (key(i)), numbered in order of first occurrence — the serial scan's
// numbering: each chunk numbers its own keys (runs of equal keys skip the map), then the chunks'
// keys are merged in chunk order and the ids remapped.  ids[i]: the cell's key id; order: the keys
// by id.  False when a chunk or the merge finds more than max_keys keys (ids then unusable).
template <class Key, class KeyFn>
static bool unique_ids(size_t n, int nth, KeyFn key, std::vector<int>& ids, std::vector<Key>& order,
                       size_t max_keys) {
  const int nch = n < 65536 ? 1 : nth;
  std::vector<std::vector<Key>> local(nch);
  std::vector<char> over(nch, 0);
  ids.resize(n);
  for_chunks(n, nch, [&](int c, size_t lo, size_t hi) {
    std::map<Key, int> uniq;
    Key last{};
    int last_id = -1;
    for (size_t i = lo; i < hi; i++) {
      const Key k = key(i);
      if (last_id >= 0 && k == last) {
        ids[i] = last_id;
        continue;
      }
      auto it = uniq.find(k);
      int id;
      if (it == uniq.end()) {
        id = (int)local[c].size();
        if ((size_t)id >= max_keys) {
          over[c] = 1;
          return;
        }
        uniq.emplace(k, id);
        local[c].push_back(k);
      } else {
        id = it->second;
      }
      ids[i] = id;
      last = k;
      last_id = id;
    }
  });
  for (int c = 0; c < nch; c++)
    if (over[c]) return false;
  std::map<Key, int> glob;
  std::vector<std::vector<int>> remap(nch);
  for (int c = 0; c < nch; c++) {
    for (const Key& k : local[c]) {
      auto it = glob.find(k);
      int g;
      if (it == glob.end()) {
        g = (int)order.size();
        if ((size_t)g >= max_keys) return false;
        glob.emplace(k, g);
        order.push_back(k);
      } else {
        g = it->second;
      }
      remap[c].push_back(g);
    }
  }
  for_chunks(n, nch, [&](int c, size_t lo, size_t hi) {
    const std::vector<int>& r = remap[c];
    for (size_t i = lo; i < hi; i++) ids[i] = r[ids[i]];
  });
  return true;
}

extern "C" {

const char* alifmm_version(void) { return "alifmm-mi355x 0.1 (gfx950)"; }

int alifmm_device_count(int* n) {
  int k = 0;
  hipError_t e = hipGetDeviceCount(&k);
  if (e != hipSuccess) k = 0;
  *n = k;
  return e == hipSuccess ? ALIFMM_OK : ALIFMM_E_HIP;
}

int alifmm_ctx_create(int device, alifmm_ctx** out) {
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return ALIFMM_E_HIP;
  if (device < 0 || device >= n) return ALIFMM_E_ARG;
  alifmm_ctx* ctx = new alifmm_ctx();
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return ALIFMM_E_HIP;
  }
  for (auto& e : ctx->ev) (void)hipEventCreate(&e);
  if (hipStreamCreateWithFlags(&ctx->fill, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_fill, hipEventDisableTiming) != hipSuccess) {
    ctx->fill = nullptr;  // fills then stay on the main stream
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->n_cu = prop.multiProcessorCount;
  // band kernel launch: cooperative (gang-scheduled: every member resident whatever else runs on
  // the device) by default; under rocprofv3 a plain launch after a residency check, because the
  // runtime's teardown of the cooperative queue at exit crashed after the profiler had finalised
  // (the plain path assumes exclusive use of the device; a member that never sees its peers stops
  // at the exchange's spin limit, error 7, and the chunk is re-run with a cooperative launch)
  ctx->coop = 1;
  for (char** e = environ; e && *e; e++)
    if (!strncmp(*e, "ROCPROF", 7) || !strncmp(*e, "ROCP_", 5)) ctx->coop = 0;
  g_live_ctx++;
  *out = ctx;
  return ALIFMM_OK;
}

// the resident sensitivity operator (alifmm_sens_op_build): it belongs to the model it was built on
static void sens_op_free(alifmm_ctx* c) {
  auto& o = c->op;
  dfree(o.row_ptr); dfree(o.col_ptr); dfree(o.col); dfree(o.row); dfree(o.cols); dfree(o.val); dfree(o.cval); dfree(o.cs);
  o = alifmm_ctx::SensOpBufs();
}

static void free_model(alifmm_ctx* c) {
  sens_op_free(c);
  dfree(c->d_veln); dfree(c->d_vm); dfree(c->d_velpn); dfree(c->d_sidx); dfree(c->d_stab); dfree(c->d_gtab);
  dfree(c->d_ptab); dfree(c->d_mid); dfree(c->d_mid8); dfree(c->d_mid8b); dfree(c->d_mtab); dfree(c->d_mslo);
  c->d_mid = nullptr;
  c->d_mid8 = nullptr;
  c->d_mid8b = nullptr;
  c->d_mtab = nullptr;
  c->d_mslo = nullptr;
  c->nmat = 0;
  c->d_veln = c->d_vm = c->d_stab = c->d_gtab = c->d_ptab = nullptr;
  c->d_velpn = c->d_sidx = nullptr;
  c->have_model = false;
}

static void free_stream_bufs(alifmm_ctx* ctx);

int alifmm_release_fields(alifmm_ctx* ctx) {
  if (!ctx) return ALIFMM_E_ARG;
  (void)hipSetDevice(ctx->device);
  for (auto& f : ctx->fields) dfree(f.d);
  ctx->fields.clear();
  free_ray_bufs(ctx);  // the ray tracer's point buffers (chunk x max_pts per coordinate) go with the fields
  release_kept_rays(ctx);
  free_stream_bufs(ctx);  // the pinned staging of streamed fields too
  return ALIFMM_OK;
}

static void destroy_team(alifmm_ctx* ctx);

int alifmm_ctx_destroy(alifmm_ctx* ctx) {
  if (!ctx) return ALIFMM_OK;
  g_live_ctx--;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  destroy_team(ctx);
  alifmm_release_fields(ctx);
  free_arena(ctx->arena);
  dfree(ctx->ho_all);
  dfree(ctx->jobs_all);
  dfree(ctx->sig_all);
  dfree(ctx->reused_all);
  ctx->ho_all = nullptr;
  ctx->jobs_all = nullptr;
  ctx->sig_all = nullptr;
  ctx->reused_all = nullptr;
  ctx->ho_last = nullptr;
  dfree(ctx->seed.ho); dfree(ctx->seed.cell); dfree(ctx->seed.close); dfree(ctx->seed.win); dfree(ctx->seed.t);
  dfree(ctx->seed.from);
  ctx->seed = alifmm_ctx::SeedBufs();
  free_ray_bufs(ctx);
  dfree(ctx->tfm.fmc); dfree(ctx->tfm.fmc64); dfree(ctx->tfm.w); dfree(ctx->tfm.tab); dfree(ctx->tfm.img);
  dfree(ctx->tfm.coh_f); dfree(ctx->tfm.coh_s);
  ctx->tfm = alifmm_ctx::TfmBufs();
  free_tfm_lsq_bufs(ctx);
  dfree(ctx->tfm_model.pix); dfree(ctx->tfm_model.refl); dfree(ctx->tfm_model.w); dfree(ctx->tfm_model.tab);
  dfree(ctx->tfm_model.out);
  ctx->tfm_model = alifmm_ctx::TfmModelBufs();
  dfree(ctx->skip.tab); dfree(ctx->skip.wiz); dfree(ctx->skip.wix); dfree(ctx->skip.row); dfree(ctx->skip.hit);
  dfree(ctx->skip.W); dfree(ctx->skip.pick);
  ctx->skip = alifmm_ctx::SkipBufs();
  {
    auto& b = ctx->sens;
    dfree(b.xy); dfree(b.off); dfree(b.cnt); dfree(b.row); dfree(b.len); dfree(b.flags); dfree(b.status); dfree(b.w);
    dfree(b.maps);
    b = alifmm_ctx::SensBufs();
  }
  dfree(ctx->solve.cell); dfree(ctx->solve.ray); dfree(ctx->solve.small);
  ctx->solve = alifmm_ctx::SolveBufs();
  for (int b = 0; b < alifmm_ctx::kPinBufs; b++) {
    if (ctx->pin[b]) (void)hipHostFree(ctx->pin[b]);
    if (ctx->pin_ev[b]) (void)hipEventDestroy(ctx->pin_ev[b]);
  }
  free_model(ctx);
  for (auto& e : ctx->ev) if (e) (void)hipEventDestroy(e);
  if (ctx->fill) {
    (void)hipStreamSynchronize(ctx->fill);
    (void)hipStreamDestroy(ctx->fill);
  }
  if (ctx->ev_fill) (void)hipEventDestroy(ctx->ev_fill);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return ALIFMM_OK;
}

const char* alifmm_last_error(alifmm_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }

int alifmm_set_option(alifmm_ctx* ctx, const char* name, double value) {
  if (!ctx || !name) return ALIFMM_E_ARG;
  if (!strcmp(name, "cdelta") && value > 0) {
    ctx->cdelta = value;
    ctx->cdelta_set = true;
  }
  else if (!strcmp(name, "r0") && value >= 0) ctx->r0 = value;
  else if (!strcmp(name, "cdelta_far") && value >= 0) ctx->cdelta_far = value;
  else if (!strcmp(name, "r_far") && value >= 0) ctx->r_far = value;
  else if (!strcmp(name, "far_sg") && value >= 0 && value == (int)value) ctx->far_sg = (int)value;
  else if (!strcmp(name, "batch") && value >= 1) ctx->batch = (int)value;
  else if (!strcmp(name, "prof")) ctx->prof = value != 0;
  else if (!strcmp(name, "coop")) ctx->coop = value != 0;
  else if (!strcmp(name, "exact_r") && value >= 0 && value <= 48) ctx->exact_r = (int)value;
  else if (!strcmp(name, "exact_lds")) ctx->exact_lds = value != 0;
  else if (!strcmp(name, "init_reuse")) ctx->init_reuse = value != 0;
  else if (!strcmp(name, "stream_out")) ctx->stream_out = value != 0;
  else if (!strcmp(name, "members") && value >= 0 && value <= af::kMaxK && value == (int)value)
    ctx->members = (int)value;
  else if (!strcmp(name, "stripe_log") && (value == 0 || (value >= 3 && value <= 12))) ctx->stripe_log = (int)value;
  else if (!strcmp(name, "xcd_local")) ctx->xcd_local = value != 0;
  else if (!strcmp(name, "tfm_chunk") && (value == 4 || value == 8 || value == 16 || value == 32)) ctx->tfm_chunk = (int)value;
  else if (!strcmp(name, "tfm_model_tile") && value >= 0 && value <= 0x7fffffff && value == (int)value)
    ctx->tfm_model_tile = (int)value;
  else if (!strcmp(name, "tfm_model_slabs") && value >= 0 && value <= 64 && value == (int)value)
    ctx->tfm_model_slabs = (int)value;
  else if (!strcmp(name, "tfm_model_rx") && (value == 1 || value == 2 || value == 4)) ctx->tfm_model_rx = (int)value;
  else if (!strcmp(name, "tfm_model_combine") && value >= 0 && value <= 64 && value == (int)value) ctx->tfm_model_combine = (int)value;
  else return fail(ctx, ALIFMM_E_ARG, "unknown option or bad value: %s=%g", name, value);
  return ALIFMM_OK;
}

int alifmm_get_option(alifmm_ctx* ctx, const char* name, double* value) {
  if (!ctx || !name || !value) return ALIFMM_E_ARG;
  if (!strcmp(name, "cdelta")) *value = band_cdelta(ctx);  // in force for the resident model
  else if (!strcmp(name, "r0")) *value = ctx->r0;
  else if (!strcmp(name, "cdelta_far")) *value = band_cdelta_far(ctx);
  else if (!strcmp(name, "mat_jump")) *value = ctx->mat_jump;
  else if (!strcmp(name, "r_far")) *value = ctx->r_far;
  else if (!strcmp(name, "far_sg")) *value = ctx->far_sg;
  else if (!strcmp(name, "batch")) *value = ctx->batch;
  else if (!strcmp(name, "exact_r")) *value = ctx->exact_r;
  else if (!strcmp(name, "exact_lds")) *value = ctx->exact_lds;
  else if (!strcmp(name, "init_reuse")) *value = ctx->init_reuse;
  else if (!strcmp(name, "init_reused")) *value = ctx->init_reused;  // last travel call: walks skipped
  else if (!strcmp(name, "stream_out")) *value = ctx->stream_out;
  else if (!strcmp(name, "stream_tail_ms")) *value = ctx->t_stream_tail;      // last travel with a host destination
  else if (!strcmp(name, "stream_fallback")) *value = (double)ctx->stream_fallback;
  else if (!strcmp(name, "exact_redo")) *value = (double)ctx->exact_redo;
  else if (!strcmp(name, "fill_wait_ms")) *value = ctx->t_fill_wait;  // last travel: fill exposed after the source init
  else if (!strcmp(name, "prof")) *value = ctx->prof;
  else if (!strcmp(name, "coop")) *value = ctx->coop;
  else if (!strcmp(name, "members")) *value = ctx->members;
  else if (!strcmp(name, "stripe_log")) *value = ctx->stripe_log;
  else if (!strcmp(name, "xcd_local")) *value = ctx->xcd_local;
  else if (!strcmp(name, "last_k")) *value = ctx->last_k;
  else if (!strcmp(name, "cap_scale")) *value = (double)ctx->cap_scale;  // read-only: x 4 per capacity retry
  else if (!strcmp(name, "n_cu")) *value = ctx->n_cu;
  else if (!strcmp(name, "vmax")) *value = ctx->vmax;  // model's fastest speed (set_model; the exact-walk stop)
  else if (!strcmp(name, "nmat")) *value = ctx->nmat;  // distinct material records (0: past the id table)
  else if (!strcmp(name, "ray_lanes")) *value = ctx->last_ray_lanes;  // lanes per ray, last find_rays
  else if (!strcmp(name, "ray_waves_per_simd")) *value = af_ray_waves_per_simd();  // ray kernel occupancy target
  // timings of the last alifmm_find_rays / alifmm_take_rays call (ms): ray kernel and point-packing
  // kernel (HIP events, summed over the launches), the whole call, and the kept points' copy-out
  else if (!strcmp(name, "ray_kernel_ms")) *value = ctx->t_ray_kernel;
  else if (!strcmp(name, "ray_pack_ms")) *value = ctx->t_ray_pack;
  else if (!strcmp(name, "find_rays_ms")) *value = ctx->t_find_rays;
  else if (!strcmp(name, "take_rays_ms")) *value = ctx->t_take_rays;
  // last alifmm_skip_pick / alifmm_skip_rays call (HIP events, ms): the gather and pair-reduction
  // kernels; the join kernel, summed over the launches (skip_rays sets the ray timings above too,
  // ray_pack_ms being 0: the join takes the packing kernel's place)
  else if (!strcmp(name, "skip_pick_ms")) *value = ctx->t_skip_pick;
  else if (!strcmp(name, "skip_join_ms")) *value = ctx->t_skip_join;
  // last alifmm_tfm call (ms): host -> device copies of the data, the weights and the slot table
  // (host clock); the delay-and-sum kernel (HIP events)
  else if (!strcmp(name, "tfm_upload_ms")) *value = ctx->t_tfm_upload;
  else if (!strcmp(name, "tfm_kernel_ms")) *value = ctx->t_tfm_kernel;
  else if (!strcmp(name, "tfm_chunk")) *value = ctx->tfm_chunk;
  // last alifmm_tfm_coh call (ms): the same two
  else if (!strcmp(name, "tfm_coh_upload_ms")) *value = ctx->t_tfm_coh_upload;
  else if (!strcmp(name, "tfm_coh_kernel_ms")) *value = ctx->t_tfm_coh_kernel;
  // last alifmm_tfm_model call (ms): the map's compaction and the host -> device copies (host clock);
  // the zeroing of the output and the kernel (HIP events).  tile / slabs: the settings (0: automatic);
  // *_used: what the last call ran with (kept apart, so that reading never pins an automatic choice)
  else if (!strcmp(name, "tfm_model_upload_ms")) *value = ctx->t_tfm_model_upload;
  else if (!strcmp(name, "tfm_model_kernel_ms")) *value = ctx->t_tfm_model_kernel;
  else if (!strcmp(name, "tfm_model_tile")) *value = ctx->tfm_model_tile;
  else if (!strcmp(name, "tfm_model_slabs")) *value = ctx->tfm_model_slabs;
  else if (!strcmp(name, "tfm_model_rx")) *value = ctx->tfm_model_rx;
  else if (!strcmp(name, "tfm_model_combine")) *value = ctx->tfm_model_combine;
  else if (!strcmp(name, "tfm_model_tile_used")) *value = ctx->tfm_model_tile_used;
  else if (!strcmp(name, "tfm_model_slabs_used")) *value = ctx->tfm_model_slabs_used;
  // last alifmm_tfm_lsq call: host -> device copies (host clock), the whole solve (device), iterations
  else if (!strcmp(name, "tfm_lsq_upload_ms")) *value = ctx->t_tfm_lsq_upload;
  else if (!strcmp(name, "tfm_lsq_kernel_ms")) *value = ctx->t_tfm_lsq_kernel;
  else if (!strcmp(name, "tfm_lsq_iters")) *value = ctx->tfm_lsq_iters;
  // last alifmm_travel_seeded call: the seed pass (uploads and fmm_seed_kernel, HIP events, ms), the
  // seeds and the close cells handed over per field
  else if (!strcmp(name, "seed_ms")) *value = ctx->t_seed;
  else if (!strcmp(name, "seed_nodes")) *value = (double)ctx->seed_nodes;
  else if (!strcmp(name, "seed_close")) *value = (double)ctx->seed_close;
  // last alifmm_ray_sens call: host -> device copies (host clock, ms), the count and fill kernels
  // (HIP events, ms), the entries (row_ptr[nrays])
  else if (!strcmp(name, "sens_upload_ms")) *value = ctx->t_sens_upload;
  else if (!strcmp(name, "sens_kernel_ms")) *value = ctx->t_sens_kernel;
  else if (!strcmp(name, "sens_entries")) *value = (double)ctx->sens_entries;
  // the resident operator: its build (the whole call, host clock, ms) and entries (0: none resident);
  // the last alifmm_sens_op_apply or _solve: device time (HIP events, ms), CGLS iterations
  else if (!strcmp(name, "solve_build_ms")) *value = ctx->t_solve_build;
  else if (!strcmp(name, "solve_kernel_ms")) *value = ctx->t_solve_kernel;
  else if (!strcmp(name, "solve_iters")) *value = ctx->solve_iters;
  else if (!strcmp(name, "sens_op_entries")) *value = ctx->op.have ? (double)ctx->op.A.entries : 0.0;
  else return fail(ctx, ALIFMM_E_ARG, "unknown option: %s", name);
  return ALIFMM_OK;
}

static af::DevModel dev_model(const alifmm_ctx* c);
int alifmm_copy_fields(alifmm_ctx* ctx, int first_slot, int n, double* dst, int dst_kind, double* gbps);

int alifmm_set_model(alifmm_ctx* ctx, int nnz, int nnx, const double* veln, const int64_t* velpn,
                     const double* vel_map, const int64_t* stif_den, const double* group_tab,
                     const double* phase_tab, int ncol, double dnx, double dnz, double gox, double goz) {
  if (!ctx || nnz < 2 || nnx < 2 || !veln || !velpn || !vel_map || !group_tab || !phase_tab || ncol < 1 ||
      ncol >= 32768)  // (the init kernels pack velpn and ncol in one int)
    return fail(ctx, ALIFMM_E_ARG, "set_model: bad arguments");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  // everything that can reject the model is checked before the resident model is released, so a
  // rejected call leaves the previous model usable
  const size_t n = (size_t)nnz * nnx;
  const int nth = host_threads();
  std::vector<int> vp(n);
  {
    std::vector<size_t> bad(std::max(1, nth), SIZE_MAX);  // per chunk: the first bad cell
    for_chunks(n, nth, [&](int c, size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; i++) {
        if (velpn[i] < 0 || velpn[i] >= ncol) {
          bad[c] = i;
          return;
        }
        vp[i] = (int)velpn[i];
      }
    });
    for (size_t b : bad)
      if (b != SIZE_MAX)
        return fail(ctx, ALIFMM_E_ARG, "velpn[%zu]=%lld outside the table", b, (long long)velpn[b]);
  }
  // unique stiffness rows (numbered in order of first occurrence)
  std::vector<int> sidx;
  std::vector<double> stab;
  if (stif_den) {
    std::vector<std::array<int64_t, 5>> rows;
    unique_ids<std::array<int64_t, 5>>(
        n, nth,
        [&](size_t i) {
          std::array<int64_t, 5> row;
          for (int k = 0; k < 5; k++) row[k] = stif_den[5 * i + k];
          return row;
        },
        sidx, rows, SIZE_MAX);
    for (const auto& row : rows)
      for (int k = 0; k < 5; k++) stab.push_back((double)row[k]);
  }
  // maximum group velocity over the model (band width scale)
  double vmax = 0;
  {
    std::vector<double> colmax(ncol, 0.0);
    for (int c = 0; c < ncol; c++)
      for (int a = 0; a <= 180; a++) colmax[c] = std::max(colmax[c], group_tab[a * ncol + c]);
    const int nrow = (int)stab.size() / 5;
    std::vector<double> rowmax(nrow, 0.0);
    for (int r = 0; r < nrow; r++)
      for (int k = 0; k <= 3600; k++)
        rowmax[r] = std::max(rowmax[r], christoffel_group_host(&stab[5 * r], 0.05 * k, 1.0));
    for (size_t i = 0; i < n; i++) {
      double v = (vp[i] != 0 || !stif_den) ? colmax[vp[i]] * vel_map[i] : rowmax[sidx[i]] * vel_map[i];
      if (std::isfinite(v)) vmax = std::max(vmax, v);
    }
  }
  if (!(vmax > 0)) return fail(ctx, ALIFMM_E_ARG, "model has no positive velocity");
  // material-interface density (band_cdelta): 4-neighbour pairs whose (veln, vel_map, velpn,
  // stiffness row) differ, over all pairs; rows spread over the host threads
  double jump = 0.0;
  {
    std::vector<long> cnt(std::max(1, nth), 0);
    auto same = [&](size_t a, size_t b) {
      return !memcmp(&veln[a], &veln[b], 8) && !memcmp(&vel_map[a], &vel_map[b], 8) && vp[a] == vp[b] &&
             (!stif_den || sidx[a] == sidx[b]);
    };
    for_chunks((size_t)nnz, n < 65536 ? 1 : std::min(nth, nnz), [&](int c, size_t z0, size_t z1) {
      long k = 0;
      for (size_t z = z0; z < z1; z++)
        for (int x = 0; x < nnx; x++) {
          const size_t i = z * nnx + x;
          if (x + 1 < nnx && !same(i, i + 1)) k++;
          if (z + 1 < (size_t)nnz && !same(i, i + nnx)) k++;
        }
      cnt[c] = k;
    }, 1);
    long k = 0;
    for (long v : cnt) k += v;
    jump = (double)k / (double)((long)(nnz - 1) * nnx + (long)nnz * (nnx - 1));
  }
  free_model(ctx);
  HIPCHK(dalloc(&ctx->d_veln, n));
  HIPCHK(dalloc(&ctx->d_vm, n));
  HIPCHK(dalloc(&ctx->d_velpn, n));
  HIPCHK(dalloc(&ctx->d_gtab, (size_t)361 * ncol));
  HIPCHK(dalloc(&ctx->d_ptab, (size_t)361 * ncol));
  HIPCHK(hipMemcpy(ctx->d_veln, veln, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->d_vm, vel_map, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->d_velpn, vp.data(), n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->d_gtab, group_tab, (size_t)361 * ncol * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->d_ptab, phase_tab, (size_t)361 * ncol * 8, hipMemcpyHostToDevice));
  if (stif_den) {
    HIPCHK(dalloc(&ctx->d_sidx, n));
    HIPCHK(dalloc(&ctx->d_stab, stab.size()));
    HIPCHK(hipMemcpy(ctx->d_sidx, sidx.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->d_stab, stab.data(), stab.size() * 8, hipMemcpyHostToDevice));
  }
  // distinct (veln, vel_map, velpn, stiffness row) records -> per-cell material ids
  {
    std::vector<af::MatRec> recs;
    std::vector<int> mid;
    std::vector<std::array<int64_t, 4>> keys;
    const bool ok = unique_ids<std::array<int64_t, 4>>(
        n, nth,
        [&](size_t i) {
          std::array<int64_t, 4> key;
          memcpy(&key[0], &veln[i], 8);
          memcpy(&key[1], &vel_map[i], 8);
          key[2] = vp[i];
          key[3] = stif_den ? sidx[i] : -1;
          return key;
        },
        mid, keys, (size_t)kMaxMatIds);
    for (const auto& key : keys) {
      af::MatRec m;
      memcpy(&m.veln, &key[0], 8);
      memcpy(&m.vm, &key[1], 8);
      m.velpn = (int)key[2];
      m.sidx = (int)key[3];
      recs.push_back(m);
    }
    if (ok) {
      HIPCHK(dalloc(&ctx->d_mid, n));
      HIPCHK(dalloc(&ctx->d_mtab, recs.size()));
      HIPCHK(hipMemcpy(ctx->d_mid, mid.data(), n * 4, hipMemcpyHostToDevice));
      if (recs.size() <= 256) {  // byte ids: 4x fewer lines per material gather in the band kernels
        std::vector<unsigned char> m8(n);
        for_chunks(n, nth, [&](int, size_t lo, size_t hi) {
          for (size_t i = lo; i < hi; i++) m8[i] = (unsigned char)mid[i];
        });
        HIPCHK(dalloc(&ctx->d_mid8, n));
        HIPCHK(hipMemcpy(ctx->d_mid8, m8.data(), n, hipMemcpyHostToDevice));
        // the same ids in 8 x 16 bricks (one 128-byte line each) for the band kernel's subgrid-1 view
        const int bp = (nnx + 15) / 16, bz = (nnz + 7) / 8;
        std::vector<unsigned char> mb((size_t)128 * bp * bz, 0);
        for_chunks((size_t)bz, std::min(nth, bz), [&](int, size_t b0, size_t b1) {  // brick rows
          for (int z = (int)b0 * 8; z < std::min(nnz, (int)b1 * 8); z++)
            for (int x = 0; x < nnx; x++)
              mb[(((size_t)(z >> 3) * bp + (x >> 4)) << 7) | ((z & 7) << 4) | (x & 15)] = m8[(size_t)z * nnx + x];
        }, n < 65536 ? SIZE_MAX : 1);
        HIPCHK(dalloc(&ctx->d_mid8b, mb.size()));
        HIPCHK(hipMemcpy(ctx->d_mid8b, mb.data(), mb.size(), hipMemcpyHostToDevice));
        ctx->mid8b_pitch = bp;
      }
      HIPCHK(hipMemcpy(ctx->d_mtab, recs.data(), recs.size() * sizeof(af::MatRec), hipMemcpyHostToDevice));
      ctx->nmat = (int)recs.size();
    }
  }
  // the small tables the source-init walk reads: another epoch when any byte of them changed
  {
    const size_t nt = (size_t)361 * ncol;
    if (ctx->tab_epoch == 0 || ctx->h_ncol != ncol || ctx->h_stab.size() != stab.size() ||
        memcmp(ctx->h_gtab.data(), group_tab, nt * 8) || memcmp(ctx->h_ptab.data(), phase_tab, nt * 8) ||
        (!stab.empty() && memcmp(ctx->h_stab.data(), stab.data(), stab.size() * 8))) {
      ctx->h_gtab.assign(group_tab, group_tab + nt);
      ctx->h_ptab.assign(phase_tab, phase_tab + nt);
      ctx->h_stab = stab;
      ctx->h_ncol = ncol;
      ctx->tab_epoch++;
    }
  }
  ctx->nstab = (int)stab.size() / 5;
  ctx->nz0 = nnz;
  ctx->nx0 = nnx;
  ctx->ncol = ncol;
  ctx->dnx = dnx;
  ctx->dnz = dnz;
  ctx->gox = gox;
  ctx->goz = goz;
  ctx->vmax = vmax;
  ctx->mat_jump = jump;
  if (ctx->nmat > 0) {  // fouds18_A() slownesses per material (band kernels' fallback)
    HIPCHK(dalloc(&ctx->d_mslo, 8 * (size_t)ctx->nmat));
    const af::DevModel M = dev_model(ctx);
    HIPCHK(af_launch_mat_slowness(&M, ctx->d_mslo, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  ctx->have_model = true;
  return ALIFMM_OK;
}

int alifmm_field_shape(alifmm_ctx* ctx, int subgrid, int* fnz, int* fnx) {
  if (!ctx || !ctx->have_model || subgrid < 1 || subgrid % 2 == 0)
    return fail(ctx, ALIFMM_E_ARG, "field_shape: no model or even subgrid %d", subgrid);
  *fnz = subgrid * (ctx->nz0 - 1) + 1;
  *fnx = subgrid * (ctx->nx0 - 1) + 1;
  return ALIFMM_OK;
}

static af::DevModel dev_model(const alifmm_ctx* c) {
  af::DevModel M;
  M.nz0 = c->nz0;
  M.nx0 = c->nx0;
  M.veln = c->d_veln;
  M.velpn = c->d_velpn;
  M.vm = c->d_vm;
  M.sidx = c->d_sidx;
  M.stab = c->d_stab;
  M.nstab = c->nstab;
  M.mid = c->d_mid;
  M.mid8 = c->d_mid8;
  M.mid8b = c->d_mid8b;
  M.mid8b_pitch = c->mid8b_pitch;
  M.mtab = c->d_mtab;
  M.nmat = c->nmat;
  M.mslo = c->d_mslo;
  M.gtab = c->d_gtab;
  M.ptab = c->d_ptab;
  M.ncol = c->ncol;
  return M;
}

// scells: cells of the row-major status S (fmm_exact_kernel's region and the mode-1 hand-over:
// subgrid > 1 only; 0 at subgrid 1, where the band kernel keeps its status in the bricked Sb)
static int ensure_arena(alifmm_ctx* ctx, int nsrc, long cells, long scells, long capL, long capC, long capS, int K,
                        long capR, long ecells, long tbc, long sbc) {
  Arena& a = ctx->arena;
  if (a.nsrc >= nsrc && a.cells >= cells && a.scells >= scells && a.capL >= capL && a.capC >= capC &&
      a.capS >= capS && a.K >= K && a.capR >= capR && a.ecells >= ecells && a.tbc >= tbc && a.sbc >= sbc)
    return ALIFMM_OK;
  // the source-init hand-overs, their signatures and jobs are no part of what a launch's geometry
  // sizes: they stay as they are (ensure_handover sizes them, for source-init launches only), so
  // that a launch of another size, member count or capacity — a seeded call's between two travel
  // calls — leaves what init_reuse vouches for and what alifmm_init_profile reads
  af::HandoverOut* const keep_ho = a.ho;
  af::InitSig* const keep_sig = a.sig;
  af::InitJob* const keep_jobs = a.jobs;
  const int keep_n = a.nho;
  a.ho = nullptr;
  a.sig = nullptr;
  a.jobs = nullptr;
  free_arena(a);
  a.ho = keep_ho;
  a.sig = keep_sig;
  a.jobs = keep_jobs;
  a.nho = keep_n;
  a.nsrc = nsrc;
  a.cells = cells;
  a.scells = scells;
  a.capL = capL;
  a.capC = capC;
  a.capS = capS;
  a.K = K;
  a.capR = capR;
  a.ecells = ecells;
  a.tbc = tbc;
  a.sbc = sbc;
  HIPCHK(dalloc(&a.Tb, (size_t)nsrc * tbc));
  HIPCHK(dalloc(&a.Sb, (size_t)nsrc * sbc));
  if (scells > 0) HIPCHK(dalloc(&a.S, (size_t)nsrc * scells));
  HIPCHK(dalloc(&a.lists, (size_t)nsrc * (4 * capL + 6 * capC)));
  HIPCHK(dalloc(&a.dlists, (size_t)nsrc * (capL + 2 * capC)));
  if (K > 1) {
    HIPCHK(dalloc(&a.rimc, (size_t)nsrc * K * 2 * capR));
    HIPCHK(dalloc(&a.rimt, (size_t)nsrc * K * 2 * capR));
  }
  HIPCHK(dalloc(&a.kx, nsrc));
  if (capS > 0) {
    HIPCHK(dalloc(&a.Ts, (size_t)nsrc * 2 * capS));
    HIPCHK(dalloc(&a.Ss, (size_t)nsrc * 2 * capS));
  }
  HIPCHK(dalloc(&a.srcs, nsrc));
  HIPCHK(dalloc(&a.dscx, nsrc));
  HIPCHK(dalloc(&a.dscz, nsrc));
  return ALIFMM_OK;
}

// hand-over slots, signatures and jobs for a source-init launch of n sources (travel_chunk's own
// launch: subgrid 1, no hand-over made elsewhere); grown only, and only here
static int ensure_handover(alifmm_ctx* ctx, int n) {
  Arena& a = ctx->arena;
  if (a.nho >= n) return ALIFMM_OK;
  if (ctx->ho_last == a.ho) {  // init profile of a chunk whose hand-overs go away
    ctx->ho_last = nullptr;
    ctx->n_ho_last = 0;
  }
  dfree(a.ho);
  dfree(a.sig);
  dfree(a.jobs);
  a.ho = nullptr;
  a.sig = nullptr;
  a.jobs = nullptr;
  a.nho = 0;
  HIPCHK(dalloc(&a.ho, n));
  HIPCHK(dalloc(&a.sig, n));
  HIPCHK(hipMemsetAsync(a.sig, 0, sizeof(af::InitSig) * n, ctx->stream));  // no slot valid
  HIPCHK(dalloc(&a.jobs, n));
  a.nho = n;
  return ALIFMM_OK;
}

int af_ensure_field(alifmm_ctx* ctx, int slot, int sg, int fz, int fx, long extra_cells) {
  if ((int)ctx->fields.size() <= slot) ctx->fields.resize(slot + 1);
  Field& f = ctx->fields[slot];
  const size_t bytes = (size_t)fz * fx * sizeof(double), need = bytes + (size_t)extra_cells * sizeof(double);
  if (f.d && f.alloc < need) {
    dfree(f.d);
    f.d = nullptr;
  }
  if (!f.d) {
    HIPCHK(hipMalloc((void**)&f.d, need));
    f.alloc = need;
  }
  f.bytes = bytes;
  f.sg = sg;
  f.nz = fz;
  f.nx = fx;
  return ALIFMM_OK;
}

// members per source of the band kernel: the largest K <= kMaxK whose grid (nsrc padded to 8, times
// K workgroups, one per CU) is co-resident, with >= 2 stripes per member
// (option "members" forces a value, still capped by residency and by the stripe count: a member
// without a stripe would only take its 1 / K share of the work lists, travel_chunk capL / K, from
// the members that own cells)
static int choose_members(const alifmm_ctx* ctx, int n, int fx) {
  const int by_cu = std::max(1, ctx->n_cu / (8 * ((n + 7) / 8)));
  if (ctx->members > 0) {
    int K = std::max(1, std::min(ctx->members, by_cu));
    // the stripe width follows K (travel_chunk) unless "stripe_log" fixes it: lower K until it fits
    for (;;) {
      const int wlog = ctx->stripe_log ? ctx->stripe_log : (K >= 16 ? 4 : K >= 8 ? 5 : 6);
      const long nstr = ((long)fx + (1L << wlog) - 1) >> wlog;
      if (K <= nstr) return K;
      K = (int)nstr;
    }
  }
  // >= 2 stripes per member at the stripe width the member count selects
  auto stripes = [&](int k) { return (long)(fx + (1 << (k >= 8 ? 4 : 6)) - 1) >> (k >= 8 ? 4 : 6); };
  int K = std::min(af::kMaxK, by_cu);
  while (K > 1 && 2L * K > stripes(K)) K--;
  return K;
}

// subgrid-1 source init (fmm_init_kernel) of n sources into ho (jobs: device scratch of n InitJobs)
// sig: the slots' signatures; reused / reused_stride: where the kernel reports each skipped walk
static int launch_source_init(alifmm_ctx* ctx, int n, const double* scx, const double* scz, af::InitJob* djobs,
                              af::HandoverOut* ho, af::InitSig* sig, int* reused, int reused_stride) {
  std::vector<af::InitJob> jobs(n);
  for (int i = 0; i < n; i++) {
    jobs[i].isx = (long)std::nearbyint((scx[i] - ctx->gox) / ctx->dnx);
    jobs[i].isz = (long)std::nearbyint((scz[i] - ctx->goz) / ctx->dnz);
    jobs[i].dnx = ctx->dnx;
    jobs[i].dnz = ctx->dnz;
    jobs[i].exact_r = ctx->exact_r;
    jobs[i].tab_epoch = ctx->tab_epoch;
    jobs[i].tstop = ctx->exact_r * ctx->dnx / ctx->vmax;
    if (jobs[i].isx < 0 || jobs[i].isx >= ctx->nx0 || jobs[i].isz < 0 || jobs[i].isz >= ctx->nz0)
      return fail(ctx, ALIFMM_E_ARG, "source %d (%g, %g) outside the grid", i, scx[i], scz[i]);
  }
  af::DevModel M = dev_model(ctx);
  HIPCHK(hipMemcpyAsync(djobs, jobs.data(), sizeof(af::InitJob) * n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(af_launch_init(&M, djobs, n, ho, sig, ctx->init_reuse, reused, reused_stride, ctx->stream));
  return ALIFMM_OK;
}

// alifmm_travel_into / alifmm_travel with a host destination: the caller's field of each source of
// a chunk, and the state of streaming them out of the band kernel (subgrid 1)
struct StreamOut {
  double* const* dst = nullptr;  // per source of the chunk
  int n = 0;
  bool active = false;  // the band launch streams (stream_setup)
  af::ts::Geometry g;
  std::atomic<int> kernel_done{0};
  std::unique_ptr<std::atomic<int>[]> missing;  // per source: a tile never arrived (copied after)
};
static int stream_setup(alifmm_ctx* ctx, StreamOut* so, int n, int K, int wlog, int fz, int fx);
static void stream_start(alifmm_ctx* ctx, StreamOut* so);
static void stream_finish(alifmm_ctx* ctx, StreamOut* so);

// travel_chunk: a plain band launch whose members were not all resident (another process held CUs);
// alifmm_travel re-runs the chunk once with a cooperative launch
static const int kRetryCoop = -100;

// one chunk of sources; returns ALIFMM_E_CAPACITY when a work list overflowed
static int travel_chunk(alifmm_ctx* ctx, int sg, int n, const double* scx, const double* scz, int first_slot, int fz,
                        int fx, float* ms_init, float* ms_band, const af::HandoverOut* pre_ho = nullptr,
                        StreamOut* so = nullptr, int* init_reused = nullptr) {
  const long cells = (long)fz * fx;
  long capL = std::min(cells, std::max(65536L, cells / 8) * ctx->cap_scale);
  long capC = capL;
  long capS = 0;
  if (sg > 1) {
    long s1 = 9L * 2 * (2L * sg + (sg - 1) / 2) + 1;             // stage-1 grid side (x9)
    long s2 = 3L * 2 * (2L * sg + (sg - 1) / 2 + 3L * sg) + 1;  // stage-2 grid side (x3)
    capS = std::max(s1 * s1, s2 * s2);
    capL = std::max(capL, std::min(capS, 262144L));
    capC = capL;
  }
  // band kernel: members per source and the stripe geometry (KGeom)
  const int K = choose_members(ctx, n, fx);
  // stripe width: 16 columns at 16 members, 32 at 8, 64 below (C4 sweeps, profiles/r6z*)
  const int wlog = ctx->stripe_log ? ctx->stripe_log : (K >= 16 ? 4 : K >= 8 ? 5 : 6), W = 1 << wlog;
  const long nstripes = (fx + W - 1) / W;
  const long capR = K > 1 ? 2L * fz * ((nstripes + K - 1) / K) + 64 : 0;
  const long ecells = K > 1 ? nstripes * 4L * fz : 0;  // per edge buffer (4 columns per stripe)
  // the band kernel's working field (af_band_tb_cells: its layout) and its edge buffers
  const long tb_cells = af_band_tb_cells(fz, fx), tbc = tb_cells + 2 * ecells, sbc = af_band_sb_cells(fz, fx);
  // the band kernel indexes the working field and both edge buffers with 32-bit cell indices
  if (tbc >= (1L << 31) - 1)
    return fail(ctx, ALIFMM_E_ARG, "travel: %d x %d grid with %ld edge cells exceeds the band kernel's 32-bit indexing",
                fz, fx, 2 * ecells);
  // the arena is sized for this chunk (reused while later chunks fit in it)
  int rc = ensure_arena(ctx, n, cells, sg > 1 ? cells : 0, capL, capC, capS, K, capR, ecells, tbc, sbc);
  if (rc) return rc;
  Arena& a = ctx->arena;
  // subgrid 1: the fields are first written by the band kernel, so their initialisation runs on
  // the fill stream beside the source-init kernel (which uses one CU per source); subgrid > 1:
  // the exact-stage kernel writes them, so in order on the main stream
  hipStream_t fs = (sg == 1 && ctx->fill) ? ctx->fill : ctx->stream;
  if (fs != ctx->stream) {  // the fill stream must not overwrite fields a previous call still reads
    HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
    HIPCHK(hipStreamWaitEvent(fs, ctx->ev[3], 0));
  }
  std::vector<af::BandSrc> hs(n);
  for (int i = 0; i < n; i++) {
    int slot = first_slot + i;
    if ((rc = af_ensure_field(ctx, slot, sg, fz, fx))) return rc;
    af::BandSrc& b = hs[i];
    memset(&b, 0, sizeof b);
    b.T = ctx->fields[slot].d;
    b.S = sg > 1 ? a.S + (size_t)i * a.scells : nullptr;
    int* base = a.lists + (size_t)i * (4 * a.capL + 6 * a.capC);
    b.Lin = base;
    b.FS = base + a.capL;
    b.A = base + 2 * a.capL;
    b.L = base + 3 * a.capL;
    b.C = base + 4 * a.capL;
    b.Cp = b.C + a.capC;
    b.D = b.C + 2 * a.capC;
    b.Rx = b.C + 3 * a.capC;
    b.Bl = b.C + 4 * a.capC;
    b.Bp = b.C + 5 * a.capC;
    double* dbase = a.dlists + (size_t)i * (a.capL + 2 * a.capC);
    b.Lt = dbase;
    b.V = dbase + a.capL;
    b.Dv = b.V + a.capC;
    b.kx = a.kx + i;
    b.Tb = a.Tb + (size_t)i * a.tbc;
    HIPCHK(hipMemsetAsync(b.Tb, 0xFF, (size_t)tbc * 8, fs));  // far: NaN (working field + edge buffers)
    b.Sb = a.Sb + (size_t)i * a.sbc;
    HIPCHK(hipMemsetAsync(b.Sb, 0xFF, (size_t)sbc * 4, fs));  // kFar = -1
    if (K > 1) {
      b.rimc = a.rimc + (size_t)i * K * 2 * capR;
      b.rimt = a.rimt + (size_t)i * K * 2 * capR;
      b.E = b.Tb + tb_cells;  // edge buffers after the working field (fmm_band_k.hip indexes both from Tb)
    }
    if (capS > 0) {
      b.Ts[0] = a.Ts + (size_t)i * 2 * a.capS;
      b.Ts[1] = b.Ts[0] + a.capS;
      b.Ss[0] = a.Ss + (size_t)i * 2 * a.capS;
      b.Ss[1] = b.Ss[0] + a.capS;
    }
    // subgrid > 1: fmm_exact_kernel writes the exact region into the result field, which must
    // start far (NaN, fields.h); subgrid 1: the band kernel's copy-out writes every cell
    if (sg > 1) HIPCHK(hipMemsetAsync(b.T, 0xFF, (size_t)cells * 8, fs));
    if (sg > 1) HIPCHK(hipMemsetAsync(b.S, 0xFF, (size_t)cells * 4, fs));  // the exact kernel's status: kFar
  }
  if (fs != ctx->stream) HIPCHK(hipEventRecord(ctx->ev_fill, fs));
  HIPCHK(hipMemcpyAsync(a.srcs, hs.data(), sizeof(af::BandSrc) * n, hipMemcpyHostToDevice, ctx->stream));
  af::DevModel M = dev_model(ctx);
  af::BandParams P;
  memset(&P, 0, sizeof P);
  P.M = M;
  P.nsrc = n;
  P.sg = sg;
  P.nz = fz;
  P.nx = fx;
  P.dnx = ctx->dnx;
  P.dnz = ctx->dnz;
  P.cdelta = band_cdelta(ctx, sg);
  P.vmax = ctx->vmax;
  P.r0 = ctx->r0;
  P.cdelta_far = sg <= ctx->far_sg ? band_cdelta_far(ctx, sg) : 0.0;
  P.r_far = ctx->r_far;
  P.capL = (int)capL;
  P.capC = (int)capC;
  P.capS = (int)capS;
  P.src = a.srcs;
  P.gox = ctx->gox;
  P.goz = ctx->goz;
  P.prof = ctx->prof;
  P.coop = ctx->coop;
  P.K = K;
  P.wlog = wlog;
  P.xcd_local = ctx->xcd_local;
  P.capR = (int)capR;
  P.ecells = ecells;
  P.tb_pitch = af_band_tb_pitch(fx);
  P.tb_cells = tb_cells;
  P.sb_pitch = af_band_sb_pitch(fx);
  P.max_steps = 200L * (fz + fx) + 100000;
  if (so) {  // stream the fields to the host while the band runs (subgrid 1)
    so->active = false;
    if (sg == 1 && ctx->stream_out && (rc = stream_setup(ctx, so, n, K, wlog, fz, fx))) return rc;
    if (so->active) {
      P.hs = static_cast<double*>(ctx->hstage);
      P.hq = ctx->hq;
      P.hcons = ctx->hcons;
      P.qcap = so->g.qcap;
      P.rslots = so->g.rslots;
      P.tr_log = so->g.trlog;
    }
  }
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  if (sg == 1) {
    if (pre_ho) {  // initialised by the travel call for all its chunks (alifmm_travel)
      P.ho = const_cast<af::HandoverOut*>(pre_ho);
    } else {
      if ((rc = ensure_handover(ctx, n))) return rc;
      // (a.srcs is uploaded above, on this stream: the kernel's word lands in the copy read back below)
      if ((rc = launch_source_init(ctx, n, scx, scz, a.jobs, a.ho, a.sig, &a.srcs[0].init_reused,
                                   (int)(sizeof(af::BandSrc) / sizeof(int)))))
        return rc;
      P.ho = a.ho;
      ctx->ho_last = a.ho;
      ctx->n_ho_last = n;
    }
    P.mode = 0;
  } else {
    for (int i = 0; i < n; i++) {
      long ix = (long)std::nearbyint((scx[i] - ctx->gox) / ctx->dnx), iz = (long)std::nearbyint((scz[i] - ctx->goz) / ctx->dnz);
      if (ix < 0 || ix >= ctx->nx0 || iz < 0 || iz >= ctx->nz0)
        return fail(ctx, ALIFMM_E_ARG, "source %d (%g, %g) outside the grid", i, scx[i], scz[i]);
    }
    HIPCHK(hipMemcpyAsync(a.dscx, scx, 8 * n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(a.dscz, scz, 8 * n, hipMemcpyHostToDevice, ctx->stream));
    P.mode = 1;
    P.scx = a.dscx;
    P.scz = a.dscz;
    // exact heap walk: both stage grids plus the fine-grid main loop out to exact_r fine nodes
    // beyond the stage-2 window (field units before the final / subgrid: coarse dnx per fine node)
    const long size2 = 2L * sg + (sg - 1) / 2 + 3L * sg;
    P.tstop = (double)(size2 + ctx->exact_r) * ctx->dnx / ctx->vmax;
    P.exact_r = ctx->exact_r;
    P.capL = (int)capL;
    P.capS = (int)capS;
    P.src = a.srcs;
    if (ctx->exact_lds && af_exact_lds_fits(sg, ctx->exact_r)) {
      HIPCHK(af_launch_exact_lds(&P, ctx->stream));
      // a heap past the LDS walk's capacity (error 9): those sources again, from scratch, with
      // the HBM walk (fmm_exact.hip)
      std::vector<af::BandSrc> chk(n);
      HIPCHK(hipMemcpyAsync(chk.data(), a.srcs, sizeof(af::BandSrc) * n, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      bool redo = false;
      for (int i = 0; i < n; i++) redo |= chk[i].err == 9;
      for (int i = 0; i < n; i++) ctx->exact_redo += chk[i].err == 9;
      if (redo) {
        for (int i = 0; i < n; i++) {
          HIPCHK(hipMemsetAsync(hs[i].T, 0xFF, (size_t)cells * 8, ctx->stream));
          HIPCHK(hipMemsetAsync(hs[i].S, 0xFF, (size_t)cells * 4, ctx->stream));
        }
        HIPCHK(hipMemcpyAsync(a.srcs, hs.data(), sizeof(af::BandSrc) * n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(af_launch_exact(&P, ctx->stream));
      }
    } else {
      HIPCHK(af_launch_exact(&P, ctx->stream));
    }
  }
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  if (fs != ctx->stream) HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_fill, 0));
  HIPCHK(hipEventRecord(ctx->ev[4], ctx->stream));  // ev[1] .. ev[4]: the fill not hidden by the source init
  HIPCHK(hipMemsetAsync(a.kx, 0, sizeof(af::KX) * n, ctx->stream));
  HIPCHK(af_launch_band_k(&P, ctx->stream));
  // the copy team takes the tiles as they arrive; joined on every return path below
  struct StreamJoin {
    alifmm_ctx* c;
    StreamOut* s;
    ~StreamJoin() {
      if (!s) return;
      // an early return: the kernel may still store into the pinned ring; it must have ended
      // before the drain stops and the next call resets or frees those buffers
      (void)hipStreamSynchronize(c->stream);
      (void)hipGetLastError();
      stream_finish(c, s);
    }
  } sjoin{ctx, nullptr};
  if (so && so->active) {
    stream_start(ctx, so);
    sjoin.s = so;
  }
  ctx->last_k = K;
  HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
  if (sg > 1)
    for (int i = 0; i < n; i++) HIPCHK(af_launch_scale(hs[i].T, cells, (double)sg, ctx->stream));
  HIPCHK(hipMemcpyAsync(hs.data(), a.srcs, sizeof(af::BandSrc) * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (sjoin.s) {
    stream_finish(ctx, so);
    sjoin.s = nullptr;
  }
  float t1 = 0, t2 = 0;
  (void)hipEventElapsedTime(&t1, ctx->ev[0], ctx->ev[1]);
  (void)hipEventElapsedTime(&t2, ctx->ev[1], ctx->ev[2]);
  *ms_init += t1;
  *ms_band += t2;
  float t3 = 0;
  (void)hipEventElapsedTime(&t3, ctx->ev[1], ctx->ev[4]);
  ctx->t_fill_wait += t3;
  if (init_reused)  // walks this chunk's own init launch skipped
    for (int i = 0; i < n; i++) *init_reused += hs[i].init_reused;
  int cap_err = 0;
  for (int i = 0; i < n; i++) {
    Field& f = ctx->fields[first_slot + i];
    for (int k = 0; k < 4; k++) f.steps[k] = hs[i].steps[k];
    f.sweeps = hs[i].nupd;
    for (int k = 0; k < 6; k++) f.prof[k] = hs[i].ph[k];
    for (int k = 0; k < 3; k++) f.prof[6 + k] = hs[i].lsum[k];
    f.prof[9] = hs[i].lmax;
    f.span[0] = hs[i].t_begin;
    f.span[1] = hs[i].t_end;
    for (int k = 0; k < 4; k++) f.prof[10 + k] = hs[i].sub[k];
    if (hs[i].err == 2) cap_err = 1;
    else if (hs[i].err == 3) return fail(ctx, ALIFMM_E_KERNEL, "source %d: init heap overflow", i);
    else if (hs[i].err == 4) return fail(ctx, ALIFMM_E_KERNEL, "source %d: stage grid capacity", i);
    else if (hs[i].err == 7 && !P.coop) return fail(ctx, kRetryCoop, "source %d: band members not co-resident", i);
    else if (hs[i].err) return fail(ctx, ALIFMM_E_KERNEL, "source %d: kernel error %d", i, hs[i].err);
  }
  if (cap_err) return fail(ctx, ALIFMM_E_CAPACITY, "work-list capacity %ld exceeded", capL);
  return ALIFMM_OK;
}

// dsts: per source, the caller's (pageable) field, or null (the fields stay resident only)
static int travel_impl(alifmm_ctx* ctx, int subgrid, int nsrc, const double* scx, const double* scz, int first_slot,
                       double* const* dsts) {
  if (!ctx || !ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "travel: no model");
  if ((long)subgrid * (ctx->nz0 - 1) + 1 >= 32768 || (long)subgrid * (ctx->nx0 - 1) + 1 >= 32768)
    return fail(ctx, ALIFMM_E_ARG, "travel: field sides must stay below 32768 nodes (packed list keys)");
  if (subgrid < 1 || subgrid % 2 == 0) return fail(ctx, ALIFMM_E_ARG, "travel: subgrid must be odd, got %d", subgrid);
  if (nsrc < 0 || first_slot < 0 || (nsrc > 0 && (!scx || !scz))) return fail(ctx, ALIFMM_E_ARG, "travel: bad args");
  HIPCHK(hipSetDevice(ctx->device));
  int fz, fx;
  alifmm_field_shape(ctx, subgrid, &fz, &fx);
  const long cells = (long)fz * fx;
  float ms_init = 0, ms_band = 0;
  // Sources per launch: at most half the CUs, so that every source gets >= 2 band members (256
  // C5 receivers on 256 CUs: one launch with one member each 927 ms, two launches of 128 with two
  // members each 810 ms, profiles/r3w_batch.json), balanced over the launches (multiples of 8)
  int chunk = std::max(1, std::min(ctx->batch, std::max(8, ctx->n_cu / 2 / 8 * 8)));
  if (nsrc > chunk) {
    const int nl = (nsrc + chunk - 1) / chunk;
    chunk = std::min(chunk, ((nsrc + nl - 1) / nl + 7) / 8 * 8);
  }
  // subgrid 1 over several launches: one source-init launch for every source of the call (the
  // init uses one CU per source; chunk by chunk it would run alone before each band launch)
  const bool pre_init = subgrid == 1 && nsrc > chunk;
  if (pre_init && ctx->n_all < nsrc) {
    if (ctx->ho_last == ctx->ho_all) {
      ctx->ho_last = nullptr;
      ctx->n_ho_last = 0;
    }
    dfree(ctx->ho_all);
    dfree(ctx->jobs_all);
    dfree(ctx->sig_all);
    dfree(ctx->reused_all);
    ctx->ho_all = nullptr;
    ctx->jobs_all = nullptr;
    ctx->sig_all = nullptr;
    ctx->reused_all = nullptr;
    ctx->n_all = 0;
    HIPCHK(dalloc(&ctx->ho_all, nsrc));
    HIPCHK(dalloc(&ctx->jobs_all, nsrc));
    HIPCHK(dalloc(&ctx->sig_all, nsrc));
    HIPCHK(dalloc(&ctx->reused_all, nsrc));
    HIPCHK(hipMemsetAsync(ctx->sig_all, 0, sizeof(af::InitSig) * nsrc, ctx->stream));  // no slot valid
    ctx->n_all = nsrc;
  }
  ctx->t_stream_tail = 0;
  ctx->stream_fallback = 0;
  ctx->exact_redo = 0;
  ctx->init_reused = 0;
  ctx->t_fill_wait = 0;
  HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
  // the call's timing events, destroyed on every return path
  struct Ev {
    hipEvent_t e = nullptr;
    ~Ev() {
      if (e) (void)hipEventDestroy(e);
    }
  } t_begin, t_end;
  HIPCHK(hipEventCreate(&t_begin.e));
  HIPCHK(hipEventCreate(&t_end.e));
  HIPCHK(hipEventRecord(t_begin.e, ctx->stream));
  const af::HandoverOut* pre = nullptr;
  if (pre_init) {
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    int rc = launch_source_init(ctx, nsrc, scx, scz, ctx->jobs_all, ctx->ho_all, ctx->sig_all, ctx->reused_all, 1);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    std::vector<int> skipped(nsrc);  // read back before the wait this path already makes
    HIPCHK(hipMemcpyAsync(skipped.data(), ctx->reused_all, sizeof(int) * nsrc, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int v : skipped) ctx->init_reused += v;
    float t = 0;
    (void)hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]);
    ms_init += t;
    pre = ctx->ho_all;
    ctx->ho_last = ctx->ho_all;
    ctx->n_ho_last = nsrc;
  }
  for (int s0 = 0; s0 < nsrc; s0 += chunk) {
    int n = std::min(chunk, nsrc - s0);
    int rc;
    StreamOut so;
    so.dst = dsts ? dsts + s0 : nullptr;
    so.n = n;
    StreamOut* sop = dsts ? &so : nullptr;
    // walks skipped by the chunk's first launch (a retry finds the hand-overs that launch wrote)
    int skipped = 0, skipped_retry = 0;
    const long cap0 = ctx->cap_scale;
    for (;;) {
      rc = travel_chunk(ctx, subgrid, n, scx + s0, scz + s0, first_slot + s0, fz, fx, &ms_init, &ms_band,
                        pre ? pre + s0 : nullptr, sop, ctx->cap_scale == cap0 ? &skipped : &skipped_retry);
      if (rc == kRetryCoop) {  // once, gang-scheduled
        const int c0 = ctx->coop;
        ctx->coop = 1;
        rc = travel_chunk(ctx, subgrid, n, scx + s0, scz + s0, first_slot + s0, fz, fx, &ms_init, &ms_band,
                          pre ? pre + s0 : nullptr, sop, &skipped_retry);
        ctx->coop = c0;
        if (rc == kRetryCoop) rc = ALIFMM_E_KERNEL;
      }
      if (rc != ALIFMM_E_CAPACITY || ctx->cap_scale * 4 > 64) break;
      ctx->cap_scale *= 4;  // retry the chunk with larger work lists
    }
    if (rc) return rc;
    ctx->init_reused += skipped;
    if (dsts) {  // fields not streamed (or a tile that never arrived): through the pinned staging ring
      for (int i = 0; i < n; i++) {
        if (so.active && !so.missing[i].load()) continue;
        if (so.active) ctx->stream_fallback++;
        rc = alifmm_copy_fields(ctx, first_slot + s0 + i, 1, dsts[s0 + i], 0, nullptr);
        if (rc) return rc;
      }
    }
  }
  HIPCHK(hipEventRecord(t_end.e, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float tot = 0;
  (void)hipEventElapsedTime(&tot, t_begin.e, t_end.e);
  ctx->t_init = ms_init;
  ctx->t_band = ms_band;
  ctx->t_total = tot;
  return ALIFMM_OK;
}

int alifmm_travel(alifmm_ctx* ctx, int subgrid, int nsrc, const double* scx, const double* scz, int first_slot,
                  double* out) {
  if (!out) return travel_impl(ctx, subgrid, nsrc, scx, scz, first_slot, nullptr);
  int fz = 0, fx = 0;
  if (ctx && ctx->have_model) alifmm_field_shape(ctx, subgrid, &fz, &fx);
  std::vector<double*> d(std::max(nsrc, 0));
  for (int i = 0; i < nsrc; i++) d[i] = out + (size_t)i * fz * fx;
  return travel_impl(ctx, subgrid, nsrc, scx, scz, first_slot, d.data());
}

int alifmm_travel_into(alifmm_ctx* ctx, int subgrid, int nsrc, const double* scx, const double* scz, int first_slot,
                       double* const* dst) {
  if (nsrc > 0 && !dst) return fail(ctx, ALIFMM_E_ARG, "travel_into: no destinations");
  for (int i = 0; i < nsrc; i++)
    if (!dst[i]) return fail(ctx, ALIFMM_E_ARG, "travel_into: destination %d is null", i);
  return travel_impl(ctx, subgrid, nsrc, scx, scz, first_slot, dst);
}

extern "C" hipError_t af_launch_seed(const af::DevModel* M, int nz, int nx, double dnx, double dnz, int nfield, int nseed,
                                     int nclose, const int* seed_cell, const int* close_cell, const int* win,
                                     const double* seed_t, const double* const* from, af::HandoverOut* out,
                                     hipStream_t stream);

// Fields from seed nodes with given times (include/alifmm.h): the host builds the geometry the
// fields share (close cells, their 5 x 5 windows into the seed list) and checks everything it can
// before any launch; fmm_seed_kernel writes one hand-over per field into the context's own buffer;
// travel_chunk runs the band from there as from a source init made elsewhere (pre_ho).
int alifmm_travel_seeded(alifmm_ctx* ctx, int nfield, int nseed, const int32_t* seed_iz, const int32_t* seed_ix,
                         const double* seed_t, const int32_t* from_slot, int first_slot, double* out) {
  if (!ctx || !ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "travel_seeded: no model");
  if (nfield < 1 || nseed < 1) return fail(ctx, ALIFMM_E_ARG, "travel_seeded: nfield %d, nseed %d", nfield, nseed);
  if (!seed_iz || !seed_ix || first_slot < 0) return fail(ctx, ALIFMM_E_ARG, "travel_seeded: bad args");
  if ((seed_t != nullptr) == (from_slot != nullptr))
    return fail(ctx, ALIFMM_E_ARG, "travel_seeded: exactly one of seed_t and from_slot must be given");
  const int nz = ctx->nz0, nx = ctx->nx0;
  if (nz >= 32768 || nx >= 32768)
    return fail(ctx, ALIFMM_E_ARG, "travel_seeded: field sides must stay below 32768 nodes (packed list keys)");
  std::vector<int> cell(nseed);
  std::unordered_map<int, int> index;  // cell -> place in the seed list
  index.reserve((size_t)nseed * 2);
  for (int k = 0; k < nseed; k++) {
    if (seed_iz[k] < 0 || seed_iz[k] >= nz || seed_ix[k] < 0 || seed_ix[k] >= nx)
      return fail(ctx, ALIFMM_E_ARG, "travel_seeded: seed %d (%d, %d) outside the %d x %d grid", k, seed_iz[k],
                  seed_ix[k], nz, nx);
    cell[k] = seed_iz[k] * nx + seed_ix[k];
    if (!index.emplace(cell[k], k).second)
      return fail(ctx, ALIFMM_E_ARG, "travel_seeded: seed %d (%d, %d) is listed twice", k, seed_iz[k], seed_ix[k]);
  }
  if (from_slot) {
    for (int i = 0; i < nfield; i++) {
      const int s = from_slot[i];
      if (s < 0 || s >= (int)ctx->fields.size() || !ctx->fields[s].d)
        return fail(ctx, ALIFMM_E_ARG, "travel_seeded: no field in from_slot %d", s);
      const Field& f = ctx->fields[s];
      if (f.sg != 1 || f.nz != nz || f.nx != nx)
        return fail(ctx, ALIFMM_E_ARG, "travel_seeded: from_slot %d holds a %d x %d field of subgrid %d, not a subgrid-1 field of the model",
                    s, f.nz, f.nx, f.sg);
      if (s >= first_slot && s < first_slot + nfield)
        return fail(ctx, ALIFMM_E_ARG, "travel_seeded: from_slot %d lies inside the destination slots %d .. %d", s,
                    first_slot, first_slot + nfield - 1);
    }
  } else {
    for (size_t k = 0; k < (size_t)nfield * nseed; k++)
      if (!(seed_t[k] >= 0.0) || seed_t[k] == INFINITY || std::signbit(seed_t[k]))
        return fail(ctx, ALIFMM_E_ARG, "travel_seeded: field %d, seed %d: time %g is not finite or is negative",
                    (int)(k / nseed), (int)(k % nseed), seed_t[k]);
  }
  // step -1's cells: every in-grid 4-neighbour of a seed that is no seed, ascending
  std::vector<int> close;
  close.reserve((size_t)nseed * 2);
  auto is_seed = [&](int z, int x) { return index.find(z * nx + x) != index.end(); };
  for (int k = 0; k < nseed; k++) {
    const int z = seed_iz[k], x = seed_ix[k];
    if (x > 0 && !is_seed(z, x - 1)) close.push_back(cell[k] - 1);
    if (x < nx - 1 && !is_seed(z, x + 1)) close.push_back(cell[k] + 1);
    if (z > 0 && !is_seed(z - 1, x)) close.push_back(cell[k] - nx);
    if (z < nz - 1 && !is_seed(z + 1, x)) close.push_back(cell[k] + nx);
  }
  std::sort(close.begin(), close.end());
  close.erase(std::unique(close.begin(), close.end()), close.end());
  const int nclose = (int)close.size();
  ctx->seed_nodes = nseed;
  ctx->seed_close = nclose;
  if ((long)nseed + nclose > af::kHandoverMax)
    return fail(ctx, ALIFMM_E_CAPACITY, "travel_seeded: %d seeds and %d close cells exceed the hand-over's %d entries",
                nseed, nclose, af::kHandoverMax);
  std::vector<int> win((size_t)nclose * 25);
  for (int j = 0; j < nclose; j++) {
    const int z = close[j] / nx, x = close[j] % nx;
    for (int o = 0; o < 25; o++) {
      const int zz = z + o / 5 - 2, xx = x + o % 5 - 2;
      int k = -1;
      if (zz >= 0 && zz < nz && xx >= 0 && xx < nx) {
        auto it = index.find(zz * nx + xx);
        if (it != index.end()) k = it->second;
      }
      win[(size_t)j * 25 + o] = k;
    }
  }
  HIPCHK(hipSetDevice(ctx->device));
  auto& sb = ctx->seed;
  HIPCHK(dgrow(&sb.ho, &sb.ho_n, (size_t)nfield));
  HIPCHK(dgrow(&sb.cell, &sb.cell_n, (size_t)nseed));
  HIPCHK(dgrow(&sb.close, &sb.close_n, (size_t)nclose));
  HIPCHK(dgrow(&sb.win, &sb.win_n, win.size()));
  ctx->t_stream_tail = 0;
  ctx->stream_fallback = 0;
  ctx->exact_redo = 0;
  ctx->init_reused = 0;
  ctx->t_fill_wait = 0;
  struct Ev {
    hipEvent_t e = nullptr;
    ~Ev() {
      if (e) (void)hipEventDestroy(e);
    }
  } t_begin, t_end;
  HIPCHK(hipEventCreate(&t_begin.e));
  HIPCHK(hipEventCreate(&t_end.e));
  HIPCHK(hipEventRecord(t_begin.e, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  HIPCHK(hipMemcpyAsync(sb.cell, cell.data(), sizeof(int) * nseed, hipMemcpyHostToDevice, ctx->stream));
  if (nclose > 0) {
    HIPCHK(hipMemcpyAsync(sb.close, close.data(), sizeof(int) * nclose, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(sb.win, win.data(), sizeof(int) * win.size(), hipMemcpyHostToDevice, ctx->stream));
  }
  std::vector<const double*> from;
  if (from_slot) {
    from.resize(nfield);
    for (int i = 0; i < nfield; i++) from[i] = ctx->fields[from_slot[i]].d;
    HIPCHK(dgrow(&sb.from, &sb.from_n, (size_t)nfield));
    HIPCHK(hipMemcpyAsync(sb.from, from.data(), sizeof(double*) * nfield, hipMemcpyHostToDevice, ctx->stream));
  } else {
    HIPCHK(dgrow(&sb.t, &sb.t_n, (size_t)nfield * nseed));
    HIPCHK(hipMemcpyAsync(sb.t, seed_t, sizeof(double) * nfield * nseed, hipMemcpyHostToDevice, ctx->stream));
  }
  // n and err of every hand-over: zeroed before, read back after the seed pass
  HIPCHK(hipMemset2DAsync(sb.ho, sizeof(af::HandoverOut), 0, 2 * sizeof(int), nfield, ctx->stream));
  af::DevModel M = dev_model(ctx);
  HIPCHK(af_launch_seed(&M, nz, nx, ctx->dnx, ctx->dnz, nfield, nseed, nclose, sb.cell, sb.close, sb.win,
                        from_slot ? nullptr : sb.t, from_slot ? sb.from : nullptr, sb.ho, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  std::vector<int> head(2 * (size_t)nfield);
  HIPCHK(hipMemcpy2DAsync(head.data(), 2 * sizeof(int), sb.ho, sizeof(af::HandoverOut), 2 * sizeof(int), nfield,
                          hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms_init = 0, ms_band = 0;
  (void)hipEventElapsedTime(&ms_init, ctx->ev[0], ctx->ev[1]);
  ctx->t_seed = ms_init;
  for (int i = 0; i < nfield; i++) {
    if (head[2 * i + 1])  // before the band launch: a negative Tmin would never accept anything
      return fail(ctx, ALIFMM_E_ARG, "travel_seeded: field %d: a seed time read from slot %d is not finite or is negative",
                  i, from_slot ? from_slot[i] : -1);
    if (head[2 * i] != nseed + nclose)
      return fail(ctx, ALIFMM_E_KERNEL, "travel_seeded: field %d: hand-over of %d entries, %d expected", i, head[2 * i],
                  nseed + nclose);
  }
  // chunks, the capacity retry and the cooperative retry as alifmm_travel (travel_impl)
  int chunk = std::max(1, std::min(ctx->batch, std::max(8, ctx->n_cu / 2 / 8 * 8)));
  if (nfield > chunk) {
    const int nl = (nfield + chunk - 1) / chunk;
    chunk = std::min(chunk, ((nfield + nl - 1) / nl + 7) / 8 * 8);
  }
  for (int s0 = 0; s0 < nfield; s0 += chunk) {
    const int n = std::min(chunk, nfield - s0);
    int rc;
    for (;;) {
      rc = travel_chunk(ctx, 1, n, nullptr, nullptr, first_slot + s0, nz, nx, &ms_init, &ms_band, sb.ho + s0);
      if (rc == kRetryCoop) {  // once, gang-scheduled
        const int c0 = ctx->coop;
        ctx->coop = 1;
        rc = travel_chunk(ctx, 1, n, nullptr, nullptr, first_slot + s0, nz, nx, &ms_init, &ms_band, sb.ho + s0);
        ctx->coop = c0;
        if (rc == kRetryCoop) rc = ALIFMM_E_KERNEL;
      }
      if (rc != ALIFMM_E_CAPACITY || ctx->cap_scale * 4 > 64) break;
      ctx->cap_scale *= 4;  // retry the chunk with larger work lists
    }
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(t_end.e, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float tot = 0;
  (void)hipEventElapsedTime(&tot, t_begin.e, t_end.e);
  ctx->t_init = ms_init;
  ctx->t_band = ms_band;
  ctx->t_total = tot;
  if (out) return alifmm_copy_fields(ctx, first_slot, nfield, out, 0, nullptr);
  return ALIFMM_OK;
}

int alifmm_get_field(alifmm_ctx* ctx, int slot, double* out) {
  if (!ctx || slot < 0 || slot >= (int)ctx->fields.size() || !ctx->fields[slot].d || !out)
    return fail(ctx, ALIFMM_E_ARG, "get_field: no field in slot %d", slot);
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(out, ctx->fields[slot].d, ctx->fields[slot].bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ALIFMM_OK;
}

// Host copy of one staged piece by a persistent team of threads (one slice each), one team per
// context (created on first use, joined by alifmm_ctx_destroy); its size is OMP_NUM_THREADS when
// set (the job's CPU share on the GPU box, 16), else up to 8.  Creating the threads per piece cost
// ~0.1 ms per 32 MiB piece (≈60 ms for a 17 GB stack).
class CopyTeam {
 public:
  explicit CopyTeam(int n) : n_(n) {
    for (int t = 1; t < n_; t++) th_.emplace_back([this, t] { run(t); });
  }
  ~CopyTeam() {
    {
      std::lock_guard<std::mutex> g(m_);
      stop_ = true;
      gen_++;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  int size() const { return n_; }
  // f(t) on the team's threads t = 1 .. size() - 1 (not the caller's); wait() joins them
  void start(std::function<void(int)> f) {
    {
      std::lock_guard<std::mutex> g(m_);
      job_ = std::move(f);
      left_ = n_ - 1;
      gen_++;
    }
    cv_.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> l(m_);
    done_.wait(l, [&] { return left_ == 0; });
  }
  void copy(char* dst, const char* src, size_t n) {
    if (n_ <= 1 || n < (4u << 20)) {
      memcpy(dst, src, n);
      return;
    }
    dst_ = dst;
    src_ = src;
    bytes_ = n;
    start([this](int t) { slice(t); });
    slice(0);
    wait();
  }

 private:
  void slice(int t) const {
    const size_t s = ((bytes_ + n_ - 1) / n_ + 4095) & ~(size_t)4095, o = (size_t)t * s;
    if (o < bytes_) memcpy(dst_ + o, src_ + o, std::min(s, bytes_ - o));
  }
  void run(int t) {
    unsigned long seen = 0;
    for (;;) {
      std::function<void(int)> f;
      {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return gen_ != seen; });
        seen = gen_;
        if (stop_) return;
        f = job_;
      }
      f(t);
      std::lock_guard<std::mutex> g(m_);
      if (--left_ == 0) done_.notify_one();
    }
  }
  int n_;
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  std::function<void(int)> job_;
  char* dst_ = nullptr;
  const char* src_ = nullptr;
  size_t bytes_ = 0;
  int left_ = 0;
  unsigned long gen_ = 0;
  bool stop_ = false;
};

static CopyTeam& copy_team(alifmm_ctx* ctx) {
  if (!ctx->team) {
    // the process's CPU share (OMP_NUM_THREADS on the GPU box, else up to 8) split over the live
    // contexts (one per GPU in update_parallel), at least two threads per team (caller + one)
    int n = (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    if (const char* e = getenv("OMP_NUM_THREADS")) {
      const int v = atoi(e);
      if (v >= 1) n = std::min(v, 32);
    }
    n = std::max(2, n / std::max(1, g_live_ctx.load()));
    ctx->team = new CopyTeam(n);
  }
  return *static_cast<CopyTeam*>(ctx->team);
}
static void destroy_team(alifmm_ctx* ctx) {
  delete static_cast<CopyTeam*>(ctx->team);
  ctx->team = nullptr;
}

static void free_stream_bufs(alifmm_ctx* ctx) {
  if (ctx->hstage) (void)hipHostFree(ctx->hstage);
  if (ctx->hq) (void)hipHostFree(ctx->hq);
  if (ctx->hcons) (void)hipHostFree(ctx->hcons);
  ctx->hstage = nullptr;
  ctx->hq = nullptr;
  ctx->hcons = nullptr;
  ctx->hstage_bytes = ctx->hq_bytes = ctx->hcons_bytes = 0;
}

static int host_buf(void** p, size_t* have, size_t need) {  // coherent pinned memory, grown on demand
  if (*have >= need) return 0;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *have = 0;
  if (hipHostMalloc(p, need, hipHostMallocCoherent) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return -1;
  }
  *have = need;
  return 0;
}

// Tile geometry (tile_stream.h) and host buffers of a streamed band launch: a ring of
// kRingSlots tile slots per member (1 GB at C4).  No geometry, no copy team or no pinned memory:
// so->active stays false (the fields are copied after the launch).
static int stream_setup(alifmm_ctx* ctx, StreamOut* so, int n, int K, int wlog, int fz, int fx) {
  so->active = false;
  if (copy_team(ctx).size() < 2 || !af::ts::plan(K, wlog, fz, fx, &so->g)) return ALIFMM_OK;
  const af::ts::Geometry& g = so->g;
  const size_t members = (size_t)n * K, tile_bytes = ((size_t)1 << g.clog()) * sizeof(double);
  const size_t qbytes = members * g.qcap * sizeof(unsigned long long);
  if (host_buf(&ctx->hstage, &ctx->hstage_bytes, members * g.rslots * tile_bytes) ||
      host_buf((void**)&ctx->hq, &ctx->hq_bytes, qbytes) ||
      host_buf((void**)&ctx->hcons, &ctx->hcons_bytes, members * sizeof(unsigned))) {
    free_stream_bufs(ctx);
    return ALIFMM_OK;
  }
  // (the previous launch that used them has completed)
  memset(ctx->hq, 0, qbytes);
  memset(ctx->hcons, 0, members * sizeof(unsigned));
  so->active = true;
  return ALIFMM_OK;
}

static void stream_start(alifmm_ctx* ctx, StreamOut* so) {
  CopyTeam& team = copy_team(ctx);
  so->kernel_done.store(0);
  so->missing.reset(new std::atomic<int>[so->n]);
  for (int i = 0; i < so->n; i++) so->missing[i].store(0);
  const int nw = team.size() - 1;
  const af::ts::Buffers b{static_cast<const double*>(ctx->hstage), ctx->hq, ctx->hcons};
  team.start([so, b, nw](int t) {
    af::ts::drain(so->g, so->n, so->dst, b, t - 1, nw,
                  [so] { return so->kernel_done.load(std::memory_order_acquire) != 0; }, so->missing.get());
  });
}

// the launch has completed (or failed): the workers finish the queues, then the team is joined
static void stream_finish(alifmm_ctx* ctx, StreamOut* so) {
  const auto t0 = std::chrono::steady_clock::now();
  so->kernel_done.store(1, std::memory_order_release);
  copy_team(ctx).wait();
  ctx->t_stream_tail += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Device -> pageable host copy of a list of segments: pieces of kPinBytes through kPinBufs pinned
// buffers; the DMA of the next pieces runs while a thread team copies the current one out of its
// buffer (alifmm_copy_fields, alifmm_take_rays)
struct D2HSeg {
  const char* src;
  char* dst;
  size_t bytes;
};
static int d2h_pageable(alifmm_ctx* ctx, const std::vector<D2HSeg>& segs) {
  const int nb = alifmm_ctx::kPinBufs;
  const size_t pb = alifmm_ctx::kPinBytes;
  size_t total = 0;
  for (const auto& g : segs) total += g.bytes;
  if (total <= kSmallD2H && !ctx->pin[0]) {
    // a small copy before the ring exists (e.g. the weld example's 8 MB of ray points): plain copies,
    // not 4 x 32 MB of fresh pinned memory (~30 ms to allocate) and a copy team
    for (const auto& g : segs) HIPCHK(hipMemcpyAsync(g.dst, g.src, g.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ALIFMM_OK;
  }
  for (int b = 0; b < nb; b++) {
    if (!ctx->pin[b]) HIPCHK(hipHostMalloc(&ctx->pin[b], pb, hipHostMallocDefault));
    if (!ctx->pin_ev[b]) HIPCHK(hipEventCreateWithFlags(&ctx->pin_ev[b], hipEventDisableTiming));
  }
  std::vector<D2HSeg> pieces;
  for (const auto& g : segs)
    for (size_t o = 0; o < g.bytes; o += pb) pieces.push_back({g.src + o, g.dst + o, std::min(pb, g.bytes - o)});
  const long np = (long)pieces.size();
  auto issue = [&](long i) -> hipError_t {
    hipError_t e = hipMemcpyAsync(ctx->pin[i % nb], pieces[i].src, pieces[i].bytes, hipMemcpyDeviceToHost, ctx->stream);
    return e == hipSuccess ? hipEventRecord(ctx->pin_ev[i % nb], ctx->stream) : e;
  };
  CopyTeam& team = copy_team(ctx);
  for (long i = 0; i < std::min<long>(nb, np); i++) HIPCHK(issue(i));
  for (long i = 0; i < np; i++) {
    HIPCHK(hipEventSynchronize(ctx->pin_ev[i % nb]));
    team.copy(pieces[i].dst, (const char*)ctx->pin[i % nb], pieces[i].bytes);
    if (i + nb < np) HIPCHK(issue(i + nb));
  }
  return ALIFMM_OK;
}

int alifmm_copy_fields(alifmm_ctx* ctx, int first_slot, int n, double* dst, int dst_kind, double* gbps) {
  if (!ctx || n < 0 || first_slot < 0 || (n > 0 && !dst) || dst_kind < 0 || dst_kind > 3)
    return fail(ctx, ALIFMM_E_ARG, "copy_fields: bad args");
  if (n == 0) return ALIFMM_OK;
  if (first_slot + n > (int)ctx->fields.size()) return fail(ctx, ALIFMM_E_ARG, "copy_fields: slots out of range");
  const size_t fb = ctx->fields[first_slot].bytes;
  for (int i = 0; i < n; i++)
    if (!ctx->fields[first_slot + i].d || ctx->fields[first_slot + i].bytes != fb)
      return fail(ctx, ALIFMM_E_ARG, "copy_fields: slot %d empty or of another shape", first_slot + i);
  HIPCHK(hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  char* out = (char*)dst;
  bool registered = false;
  if (dst_kind == 3) {  // pageable destination registered for this copy: the DMA writes it directly
    HIPCHK(hipHostRegister(dst, (size_t)n * fb, hipHostRegisterDefault));
    registered = true;
    dst_kind = 1;
  }
  if (dst_kind != 0) {  // one DMA per field (device -> device, or into host memory the DMA can write)
    const hipMemcpyKind kind = dst_kind == 2 ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; i++)
      e = hipMemcpyAsync(out + (size_t)i * fb, ctx->fields[first_slot + i].d, fb, kind, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (registered) (void)hipHostUnregister(dst);
    if (e != hipSuccess || es != hipSuccess)
      return fail(ctx, ALIFMM_E_HIP, "copy_fields: %s", hipGetErrorString(e != hipSuccess ? e : es));
  } else {
    std::vector<D2HSeg> segs(n);
    for (int i = 0; i < n; i++) segs[i] = {(const char*)ctx->fields[first_slot + i].d, out + (size_t)i * fb, fb};
    const int rc = d2h_pageable(ctx, segs);
    if (rc) return rc;
  }
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (gbps) *gbps = dt > 0 ? (double)fb * n / dt / 1e9 : 0.0;
  return ALIFMM_OK;
}

int alifmm_source_stats(alifmm_ctx* ctx, int slot, int64_t* steps4, int64_t* cell_sweeps) {
  if (!ctx || slot < 0 || slot >= (int)ctx->fields.size()) return fail(ctx, ALIFMM_E_ARG, "stats: bad slot");
  if (steps4)
    for (int k = 0; k < 4; k++) steps4[k] = ctx->fields[slot].steps[k];
  if (cell_sweeps) *cell_sweeps = ctx->fields[slot].sweeps;
  return ALIFMM_OK;
}

int alifmm_band_profile(alifmm_ctx* ctx, int slot, int64_t* out14) {
  if (!ctx || slot < 0 || slot >= (int)ctx->fields.size() || !out14) return fail(ctx, ALIFMM_E_ARG, "band_profile: bad slot");
  for (int k = 0; k < 14; k++) out14[k] = ctx->fields[slot].prof[k];
  return ALIFMM_OK;
}

int alifmm_band_span(alifmm_ctx* ctx, int slot, int64_t* out2) {
  if (!ctx || slot < 0 || slot >= (int)ctx->fields.size() || !out2) return fail(ctx, ALIFMM_E_ARG, "band_span: bad slot");
  out2[0] = ctx->fields[slot].span[0];
  out2[1] = ctx->fields[slot].span[1];
  return ALIFMM_OK;
}

int alifmm_init_profile(alifmm_ctx* ctx, int i, int64_t* out16) {
  if (!ctx || !out16 || i < 0 || i >= ctx->n_ho_last || !ctx->ho_last)
    return fail(ctx, ALIFMM_E_ARG, "init_profile: bad index");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpy(out16, &ctx->ho_last[i].prof[0], 16 * sizeof(long long), hipMemcpyDeviceToHost));
  return ALIFMM_OK;
}

int alifmm_last_timing(alifmm_ctx* ctx, double* init_ms, double* band_ms, double* total_ms) {
  if (!ctx) return ALIFMM_E_ARG;
  if (init_ms) *init_ms = ctx->t_init;
  if (band_ms) *band_ms = ctx->t_band;
  if (total_ms) *total_ms = ctx->t_total;
  return ALIFMM_OK;
}

// the ray tracer's work buffers hold `rays` rays of max_pts points (kept across calls, regrown for a larger launch)
static int ensure_ray_bufs(alifmm_ctx* ctx, int rays, int max_pts) {
  auto& rb = ctx->rb;
  if (rb.rays >= rays && rb.pts >= (size_t)rays * max_pts) return ALIFMM_OK;
  free_ray_bufs(ctx);
  HIPCHK(dalloc(&rb.rx, (size_t)rays * max_pts));
  HIPCHK(dalloc(&rb.ry, (size_t)rays * max_pts));
  HIPCHK(dalloc(&rb.t, rays));
  HIPCHK(dalloc(&rb.len, rays));
  HIPCHK(dalloc(&rb.flags, rays));
  HIPCHK(dalloc(&rb.jobs, rays));
  HIPCHK(dalloc(&rb.off, rays));
  rb.rays = rays;
  rb.pts = (size_t)rays * max_pts;
  return ALIFMM_OK;
}

// device-kept chunks -> per-ray host staging (the kept budget is spent): the chunks hold the rays
// ids[0], ids[1], ... in order, lens[id] points each; the chunks are freed
static hipError_t spill_kept_rays(alifmm_ctx* ctx, const int* ids, const std::vector<int32_t>& lens,
                                  std::vector<std::vector<double>>& staged) {
  staged.assign(lens.size(), {});
  size_t r = 0;
  for (auto& k : ctx->kept_dev) {
    std::vector<double> h(2 * (size_t)k.npts);
    hipError_t e = hipMemcpy(h.data(), k.d, 16 * (size_t)k.npts, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    size_t o = 0;
    while (o < (size_t)k.npts) {
      const int id = ids[r++];
      staged[id].assign(h.begin() + 2 * o, h.begin() + 2 * (o + lens[id]));
      o += lens[id];
    }
  }
  for (auto& k : ctx->kept_dev) dfree(k.d);
  ctx->kept_dev.clear();
  ctx->kept_pts = 0;
  return hipSuccess;
}

int alifmm_find_rays(alifmm_ctx* ctx, int npairs, const int32_t* field_slot, const double* src_xy,
                     const double* rec_xy, double* times, int32_t* ray_len, int32_t* flags, double* ray_xy,
                     int64_t ray_xy_cap) {
  if (!ctx || !ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "find_rays: no model");
  if (npairs <= 0) return ALIFMM_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const auto t_call = std::chrono::steady_clock::now();
  ctx->t_ray_kernel = ctx->t_ray_pack = 0;
  const int max_pts = 5 * (ctx->nz0 + ctx->nx0);
  // group rays by subgrid (one launch per subgrid size present)
  std::map<int, std::vector<int>> by_sg;
  for (int k = 0; k < npairs; k++) {
    int s = field_slot[k];
    if (s < 0 || s >= (int)ctx->fields.size() || !ctx->fields[s].d)
      return fail(ctx, ALIFMM_E_ARG, "find_rays: ray %d refers to empty slot %d", k, s);
    by_sg[ctx->fields[s].sg].push_back(k);
  }
  for (auto& g : by_sg)
    if (6 * g.first + 3 > kMaxRayCand)  // the plane search keeps <= kMaxRayCand candidates per ray (rays.hip)
      return fail(ctx, ALIFMM_E_ARG, "find_rays: subgrid %d has %d plane candidates (> %d supported)", g.first,
                  6 * g.first + 3, kMaxRayCand);
  // chunk of rays per launch; the point buffers (chunk x max_pts per coordinate) are sized to the
  // request and kept in the context for the next call
  // Rays per launch: wavefronts for every SIMD at the ray kernel's occupancy (af_ray_waves_per_simd;
  // 8 192 rays at 16 lanes per ray and 2 wavefronts per SIMD), balanced over the launches, with the
  // point buffers within a quarter of the free device memory.
  int chunk = 8192;
  int ray_packed = 0;
  size_t keep_budget = SIZE_MAX;  // device bytes the kept points of this call may hold (a quarter of the free memory)
  {
    // 9-lane groups (7 rays per wavefront) only for requests that fill the device with them: fewer
    // rays in 16-lane groups give every SIMD its wavefronts (8 192 rays: 0.130 s vs 0.173 s,
    // profiles/r5e)
    const long fill9 = (long)std::max(ctx->n_cu, 1) * 4 * af_ray_waves_per_simd() * (64 / 9);
    ray_packed = npairs >= fill9 ? 1 : 0;
    int rays_per_wave = 64;
    for (auto& g : by_sg) rays_per_wave = std::min(rays_per_wave, 64 / af_ray_group_lanes(g.first, ray_packed));
    const long target = (long)std::max(ctx->n_cu, 1) * 4 * af_ray_waves_per_simd() * rays_per_wave;
    size_t free_b = 0, total_b = 0;
    long by_mem = target;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      by_mem = (long)(free_b / 4 / ((size_t)max_pts * 2 * sizeof(double) + 64));
      keep_budget = free_b / 4;
    }
    const long cmax = std::max(1024L, std::min(target, by_mem));
    const long nlaunch = (npairs + cmax - 1) / cmax;
    chunk = (int)((npairs + nlaunch - 1) / nlaunch);
  }
  chunk = std::min(chunk, npairs);
  auto& rb = ctx->rb;
  if (int rc = ensure_ray_bufs(ctx, chunk, max_pts)) return rc;
  double *d_rx = rb.rx, *d_ry = rb.ry, *d_t = rb.t, *d_packed = nullptr;
  int *d_len = rb.len, *d_flags = rb.flags;
  af::RayJob* d_jobs = rb.jobs;
  long long* d_off = rb.off;
  int rc = ALIFMM_OK;
  auto cleanup = [&]() { dfree(d_packed); };
  // an error return also drops the points kept so far (kept_pts then matches no ray list)
#define RCHK(call)                                                                        \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      cleanup();                                                                          \
      release_kept_rays(ctx);                                                             \
      return fail(ctx, ALIFMM_E_HIP, "%s: %s", #call, hipGetErrorString(e_));             \
    }                                                                                     \
  } while (0)
  std::vector<int64_t> offsets(npairs + 1, 0);
  std::vector<int32_t> lens(npairs, 0);
  std::vector<double> tms(npairs, 0.0);
  std::vector<int32_t> flg(npairs, 0);
  // pass 1: trace, lengths
  struct Pending { std::vector<int> ids; };
  std::vector<std::pair<int, std::vector<int>>> groups(by_sg.begin(), by_sg.end());
  // Rays are traced chunk by chunk; packed points are written after lengths are known (pass 2 re-traces
  // nothing: each chunk is packed right after its trace, at offsets relative to the ray order below).
  std::vector<int> order;
  for (auto& g : groups) order.insert(order.end(), g.second.begin(), g.second.end());
  // offsets follow the caller's ray order; we first trace everything (times/lengths), packing each
  // chunk into a host staging area keyed by ray id.
  const bool keep = !ray_xy && ray_xy_cap == ALIFMM_KEEP_RAYS;
  // one subgrid (the usual case): the rays are traced in the caller's order, so the kept points
  // stay on the device, chunk after chunk, and alifmm_take_rays copies them out once
  // (while the kept bytes stay within keep_budget; past it the kept chunks move to host staging)
  bool dev_keep = keep && groups.size() == 1;
  release_kept_rays(ctx);
  std::vector<std::vector<double>> staged(((ray_xy || keep) && !dev_keep) ? npairs : 0);
  size_t kept_bytes = 0;
  // device-kept chunks -> per-ray host staging (rays ids[0 .. ndone-1] of the single group, in order)
  auto spill_kept = [&](const std::vector<int>& ids) -> hipError_t {
    dev_keep = false;
    return spill_kept_rays(ctx, ids.data(), lens, staged);
  };
  for (auto& g : groups) {
    const int sg = g.first;
    const auto& ids = g.second;
    const Field& f0 = ctx->fields[field_slot[ids[0]]];
    for (size_t c0 = 0; c0 < ids.size(); c0 += chunk) {
      int n = (int)std::min<size_t>(chunk, ids.size() - c0);
      std::vector<af::RayJob> jobs(n);
      for (int i = 0; i < n; i++) {
        int k = ids[c0 + i];
        const Field& f = ctx->fields[field_slot[k]];
        jobs[i].ttf = f.d;
        jobs[i].sx = src_xy[2 * k];
        jobs[i].sy = src_xy[2 * k + 1];
        jobs[i].rx = rec_xy[2 * k];
        jobs[i].ry = rec_xy[2 * k + 1];
        if (f.nz != f0.nz || f.nx != f0.nx) {
          cleanup();
          release_kept_rays(ctx);
          return fail(ctx, ALIFMM_E_ARG, "find_rays: mixed field shapes for subgrid %d", sg);
        }
      }
      RCHK(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(af::RayJob) * n, hipMemcpyHostToDevice, ctx->stream));
      af::RayParams P;
      memset(&P, 0, sizeof P);
      P.M = dev_model(ctx);
      P.fnz = f0.nz;
      P.fnx = f0.nx;
      P.sg = sg;
      P.dnx = ctx->dnx;
      P.nrays = n;
      P.max_pts = max_pts;
      P.jobs = d_jobs;
      P.ray_x = d_rx;
      P.ray_y = d_ry;
      P.ray_len = d_len;
      P.times = d_t;
      P.flags = d_flags;
      P.glanes = af_ray_group_lanes(sg, ray_packed);
      ctx->last_ray_lanes = P.glanes;
      RCHK(hipEventRecord(ctx->ev[0], ctx->stream));
      RCHK(af_launch_rays(&P, ctx->stream));
      RCHK(hipEventRecord(ctx->ev[1], ctx->stream));
      std::vector<double> t(n);
      std::vector<int> l(n), fl(n);
      RCHK(hipMemcpyAsync(t.data(), d_t, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
      RCHK(hipMemcpyAsync(l.data(), d_len, 4 * n, hipMemcpyDeviceToHost, ctx->stream));
      RCHK(hipMemcpyAsync(fl.data(), d_flags, 4 * n, hipMemcpyDeviceToHost, ctx->stream));
      RCHK(hipStreamSynchronize(ctx->stream));
      {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]);
        ctx->t_ray_kernel += ms;
      }
      for (int i = 0; i < n; i++) {
        int k = ids[c0 + i];
        tms[k] = t[i];
        lens[k] = l[i];
        flg[k] = fl[i];
      }
      if (ray_xy || keep) {
        std::vector<long long> off(n + 1, 0);
        for (int i = 0; i < n; i++) off[i + 1] = off[i] + l[i];
        dfree(d_packed);
        d_packed = nullptr;
        RCHK(dalloc(&d_packed, (size_t)2 * std::max<long long>(off[n], 1)));
        RCHK(hipMemcpyAsync(d_off, off.data(), 8 * n, hipMemcpyHostToDevice, ctx->stream));
        RCHK(hipEventRecord(ctx->ev[2], ctx->stream));
        RCHK(af_launch_pack_rays(d_rx, d_ry, d_len, d_off, n, max_pts, d_packed, ctx->stream));
        RCHK(hipEventRecord(ctx->ev[3], ctx->stream));
        RCHK(hipEventSynchronize(ctx->ev[3]));
        {
          float ms = 0;
          (void)hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]);
          ctx->t_ray_pack += ms;
        }
        if (dev_keep && kept_bytes + 16 * (size_t)off[n] > keep_budget) RCHK(spill_kept(ids));
        if (dev_keep) {  // the chunk's packed points stay on the device (the context owns them now)
          kept_bytes += 16 * (size_t)off[n];
          ctx->kept_dev.push_back({d_packed, (int64_t)off[n]});
          ctx->kept_pts += off[n];
          d_packed = nullptr;
          continue;
        }
        std::vector<double> packed(2 * off[n]);
        RCHK(hipMemcpyAsync(packed.data(), d_packed, 16 * off[n], hipMemcpyDeviceToHost, ctx->stream));
        RCHK(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < n; i++)
          staged[ids[c0 + i]].assign(packed.begin() + 2 * off[i], packed.begin() + 2 * off[i + 1]);
      }
    }
  }
  for (int k = 0; k < npairs; k++) offsets[k + 1] = offsets[k] + lens[k];
  if (ray_xy && offsets[npairs] > ray_xy_cap) rc = fail(ctx, ALIFMM_E_ARG, "find_rays: ray_xy capacity %lld < %lld",
                                                      (long long)ray_xy_cap, (long long)offsets[npairs]);
  if (!rc) {
    for (int k = 0; k < npairs; k++) {
      times[k] = tms[k];
      ray_len[k] = lens[k];
      if (flags) flags[k] = flg[k];
      if (ray_xy) std::copy(staged[k].begin(), staged[k].end(), ray_xy + 2 * offsets[k]);
    }
    if (keep && !dev_keep) {
      ctx->kept_rays.swap(staged);
      ctx->kept_pts = offsets[npairs];
    }
  }
  if (rc || (dev_keep && ctx->kept_pts != offsets[npairs])) {
    release_kept_rays(ctx);
    if (!rc) rc = fail(ctx, ALIFMM_E_KERNEL, "find_rays: kept points do not add up to the ray lengths");
  }
  cleanup();
  ctx->t_find_rays = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
  // point buffers above kRayBufKeepBytes (C4: 8192 rays x 40 960 points x 16 B = 5.4 GB) are not kept
  // between calls, so they do not hold device memory that later travel / arena allocations need
  if (rb.pts * 2 * sizeof(double) > kRayBufKeepBytes) free_ray_bufs(ctx);
  return rc;
}

int alifmm_take_rays(alifmm_ctx* ctx, double* ray_xy, int64_t ray_xy_cap, int64_t* n_points) {
  if (!ctx) return ALIFMM_E_ARG;
  if (n_points) *n_points = ctx->kept_pts;
  if (!ray_xy) return ALIFMM_OK;  // size query
  if (ray_xy_cap < ctx->kept_pts)
    return fail(ctx, ALIFMM_E_ARG, "take_rays: ray_xy capacity %lld < %lld", (long long)ray_xy_cap,
                (long long)ctx->kept_pts);
  int64_t off = 0;
  const auto t_call = std::chrono::steady_clock::now();
  auto done = [&](int rc) {
    ctx->t_take_rays = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    return rc;
  };
  if (!ctx->kept_dev.empty()) {  // device-resident chunks: one pass through the pinned ring
    std::vector<D2HSeg> segs;
    for (auto& k : ctx->kept_dev) {
      segs.push_back({(const char*)k.d, (char*)(ray_xy + 2 * off), (size_t)k.npts * 16});
      off += k.npts;
    }
    HIPCHK(hipSetDevice(ctx->device));
    const int rc = d2h_pageable(ctx, segs);
    release_kept_rays(ctx);
    return done(rc);
  }
  for (auto& r : ctx->kept_rays) {
    std::copy(r.begin(), r.end(), ray_xy + 2 * off);
    off += (int64_t)r.size() / 2;
  }
  release_kept_rays(ctx);
  return done(ALIFMM_OK);
}

// ---- back-wall echo paths between element pairs (skip_pairs.hip) ----
// the checked request of alifmm_skip_pick / alifmm_skip_rays and its picks
struct SkipRequest {
  int sg = 0, fnz = 0, fnx = 0;
  std::vector<int32_t> hit;
  std::vector<double> pick;
};

// checks (ALIFMM_E_ARG, nothing launched), then the gather and the pair reduction; the picks on the host
static int skip_pick_run(alifmm_ctx* ctx, const char* what, int npairs, const int32_t* slot_a, const int32_t* slot_b,
                         int nw, const int32_t* w_iz, const int32_t* w_ix, bool rays, SkipRequest& R) {
  if (!slot_a || !slot_b) return fail(ctx, ALIFMM_E_ARG, "%s: slot_a or slot_b is NULL", what);
  if (!w_iz || !w_ix) return fail(ctx, ALIFMM_E_ARG, "%s: w_iz or w_ix is NULL", what);
  // the distinct slots of the request, in order of first use: row r of W belongs to slots[r]
  std::unordered_map<int, int> row_of;
  std::vector<int> slots;
  std::vector<int32_t> rows(2 * (size_t)npairs);
  for (int k = 0; k < 2 * npairs; k++) {
    const int s = k < npairs ? slot_a[k] : slot_b[k - npairs];
    if (s < 0 || s >= (int)ctx->fields.size() || !ctx->fields[s].d)
      return fail(ctx, ALIFMM_E_ARG, "%s: pair %d refers to empty slot %d", what, k % npairs, s);
    auto it = row_of.find(s);
    if (it == row_of.end()) {
      it = row_of.emplace(s, (int)slots.size()).first;
      slots.push_back(s);
    }
    rows[k] = it->second;
  }
  const Field& f0 = ctx->fields[slots[0]];
  for (int s : slots) {
    const Field& f = ctx->fields[s];
    if (f.sg != f0.sg) return fail(ctx, ALIFMM_E_ARG, "%s: mixed subgrids %d and %d (slots %d and %d)", what, f0.sg, f.sg, slots[0], s);
    if (f.nz != f0.nz || f.nx != f0.nx)
      return fail(ctx, ALIFMM_E_ARG, "%s: mixed field shapes (slots %d and %d)", what, slots[0], s);
  }
  for (int q = 0; q < nw; q++)
    if (w_iz[q] < 0 || w_iz[q] >= f0.nz || w_ix[q] < 0 || w_ix[q] >= f0.nx)
      return fail(ctx, ALIFMM_E_ARG, "%s: reflector node %d (%d, %d) outside the %d x %d field", what, q, w_iz[q], w_ix[q],
                  f0.nz, f0.nx);
  if (rays && 6 * f0.sg + 3 > kMaxRayCand)
    return fail(ctx, ALIFMM_E_ARG, "%s: subgrid %d has %d plane candidates (> %d supported)", what, f0.sg, 6 * f0.sg + 3,
                kMaxRayCand);
  if (slots.size() > 65535) return fail(ctx, ALIFMM_E_ARG, "%s: %zu distinct slots (> 65535)", what, slots.size());
  R.sg = f0.sg;
  R.fnz = f0.nz;
  R.fnx = f0.nx;
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::SkipBufs& B = ctx->skip;
  const size_t np = (size_t)npairs, nf = slots.size();
  HIPCHK(dgrow(&B.tab, &B.tab_n, nf));
  HIPCHK(dgrow(&B.wiz, &B.wiz_n, (size_t)nw));
  HIPCHK(dgrow(&B.wix, &B.wix_n, (size_t)nw));
  HIPCHK(dgrow(&B.row, &B.row_n, 2 * np));
  HIPCHK(dgrow(&B.hit, &B.hit_n, np));
  HIPCHK(dgrow(&B.pick, &B.pick_n, np));
  HIPCHK(dgrow(&B.W, &B.W_n, nf * (size_t)nw));
  std::vector<const double*> tab(nf);
  for (size_t r = 0; r < nf; r++) tab[r] = ctx->fields[slots[r]].d;
  HIPCHK(hipMemcpyAsync(B.tab, tab.data(), nf * sizeof(double*), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(B.wiz, w_iz, (size_t)nw * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(B.wix, w_ix, (size_t)nw * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(B.row, rows.data(), 2 * np * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  HIPCHK(af_launch_skip_pick(B.tab, (int)nf, B.wiz, B.wix, f0.nx, nw, B.W, B.row, B.row + np, npairs, B.pick, B.hit,
                             ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  R.hit.resize(np);
  R.pick.resize(np);
  HIPCHK(hipMemcpyAsync(R.hit.data(), B.hit, np * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(R.pick.data(), B.pick, np * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));  // the staging vectors above live until here
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]);
  ctx->t_skip_pick = ms;
  return ALIFMM_OK;
}

static int skip_check_counts(alifmm_ctx* ctx, const char* what, int npairs, int nw) {
  if (!ctx) return ALIFMM_E_ARG;
  if (!ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "%s: no model", what);
  if (npairs < 0) return fail(ctx, ALIFMM_E_ARG, "%s: npairs %d", what, npairs);
  if (nw < 1) return fail(ctx, ALIFMM_E_ARG, "%s: nw %d", what, nw);
  return ALIFMM_OK;
}

int alifmm_skip_pick(alifmm_ctx* ctx, int npairs, const int32_t* slot_a, const int32_t* slot_b, int nw,
                     const int32_t* w_iz, const int32_t* w_ix, double* pick_time, int32_t* hit) {
  if (int rc = skip_check_counts(ctx, "skip_pick", npairs, nw)) return rc;
  if (npairs == 0) return ALIFMM_OK;
  if (!pick_time || !hit) return fail(ctx, ALIFMM_E_ARG, "skip_pick: pick_time or hit is NULL");
  ctx->t_skip_pick = ctx->t_skip_join = 0;
  SkipRequest R;
  if (int rc = skip_pick_run(ctx, "skip_pick", npairs, slot_a, slot_b, nw, w_iz, w_ix, false, R)) return rc;
  std::copy(R.hit.begin(), R.hit.end(), hit);
  std::copy(R.pick.begin(), R.pick.end(), pick_time);
  return ALIFMM_OK;
}

int alifmm_skip_rays(alifmm_ctx* ctx, int npairs, const int32_t* slot_a, const int32_t* slot_b, const double* a_xy,
                     const double* b_xy, int nw, const int32_t* w_iz, const int32_t* w_ix, double* pick_time,
                     int32_t* hit, double* times, int32_t* ray_len, int32_t* flags, double* ray_xy,
                     int64_t ray_xy_cap) {
  if (int rc = skip_check_counts(ctx, "skip_rays", npairs, nw)) return rc;
  if (npairs == 0) return ALIFMM_OK;
  if (!a_xy || !b_xy) return fail(ctx, ALIFMM_E_ARG, "skip_rays: a_xy or b_xy is NULL");
  if (!times || !ray_len) return fail(ctx, ALIFMM_E_ARG, "skip_rays: times or ray_len is NULL");
  const auto t_call = std::chrono::steady_clock::now();
  ctx->t_skip_pick = ctx->t_skip_join = 0;
  SkipRequest R;
  if (int rc = skip_pick_run(ctx, "skip_rays", npairs, slot_a, slot_b, nw, w_iz, w_ix, true, R)) return rc;
  ctx->t_ray_kernel = ctx->t_ray_pack = 0;
  const int max_pts = 5 * (ctx->nz0 + ctx->nx0);  // per leg; a joined ray holds up to 2 max_pts - 1
  // Pairs per launch: two legs a pair, the legs sized as alifmm_find_rays sizes its rays (wavefronts for
  // every SIMD at the ray kernel's occupancy, the point buffers within a quarter of the free memory);
  // 9-lane groups when the legs fill the device with them
  const long fill9 = (long)std::max(ctx->n_cu, 1) * 4 * af_ray_waves_per_simd() * (64 / 9);
  const int ray_packed = 2L * npairs >= fill9 ? 1 : 0;
  const int glanes = af_ray_group_lanes(R.sg, ray_packed);
  size_t keep_budget = SIZE_MAX;
  int chunk = npairs;
  {
    const long target = (long)std::max(ctx->n_cu, 1) * 4 * af_ray_waves_per_simd() * (64 / glanes);
    size_t free_b = 0, total_b = 0;
    long by_mem = target;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      by_mem = (long)(free_b / 4 / ((size_t)max_pts * 2 * sizeof(double) + 64));
      keep_budget = free_b / 4;
    }
    const long cmax = std::max(1024L, std::min(target, by_mem)) / 2;
    const long nlaunch = (npairs + cmax - 1) / cmax;
    chunk = (int)std::min<long>((npairs + nlaunch - 1) / nlaunch, npairs);
  }
  auto& rb = ctx->rb;
  if (int rc = ensure_ray_bufs(ctx, 2 * chunk, max_pts)) return rc;
  double* d_packed = nullptr;
  // an error return also drops the points kept so far (kept_pts then matches no ray list)
#define SCHK(call)                                                            \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess) {                                                   \
      dfree(d_packed);                                                        \
      release_kept_rays(ctx);                                                 \
      return fail(ctx, ALIFMM_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    }                                                                         \
  } while (0)
  std::vector<int32_t> lens(npairs, 0), flg(npairs, 0);
  std::vector<double> tms(npairs, 0.0);
  std::vector<int> ids(npairs);
  for (int k = 0; k < npairs; k++) ids[k] = k;
  const bool keep = !ray_xy && ray_xy_cap == ALIFMM_KEEP_RAYS;
  // the pairs are traced in the caller's order, so kept points stay on the device, chunk after chunk
  // (within keep_budget; past it the kept chunks move to host staging), as after alifmm_find_rays
  bool dev_keep = keep;
  release_kept_rays(ctx);
  std::vector<std::vector<double>> staged(ray_xy ? npairs : 0);
  size_t kept_bytes = 0;
  const af::DevModel M = dev_model(ctx);
  for (int c0 = 0; c0 < npairs; c0 += chunk) {
    const int n = std::min(chunk, npairs - c0);
    // the chunk's pairs with a hit: pair live[p] has legs 2 p (to a) and 2 p + 1 (to b) of the launch
    std::vector<int> live;
    std::vector<af::RayJob> jobs;
    for (int i = 0; i < n; i++) {
      const int k = c0 + i, h = R.hit[k];
      if (h < 0) {
        flg[k] = 8;
        continue;
      }
      live.push_back(k);
      af::RayJob J;
      J.sx = (double)w_ix[h];
      J.sy = (double)w_iz[h];
      J.ttf = ctx->fields[slot_a[k]].d;
      J.rx = a_xy[2 * k];
      J.ry = a_xy[2 * k + 1];
      jobs.push_back(J);
      J.ttf = ctx->fields[slot_b[k]].d;
      J.rx = b_xy[2 * k];
      J.ry = b_xy[2 * k + 1];
      jobs.push_back(J);
    }
    const int m = (int)live.size();
    if (!m) continue;
    SCHK(hipMemcpyAsync(rb.jobs, jobs.data(), sizeof(af::RayJob) * 2 * m, hipMemcpyHostToDevice, ctx->stream));
    af::RayParams P;
    memset(&P, 0, sizeof P);
    P.M = M;
    P.fnz = R.fnz;
    P.fnx = R.fnx;
    P.sg = R.sg;
    P.dnx = ctx->dnx;
    P.nrays = 2 * m;
    P.max_pts = max_pts;
    P.jobs = rb.jobs;
    P.ray_x = rb.rx;
    P.ray_y = rb.ry;
    P.ray_len = rb.len;
    P.times = rb.t;
    P.flags = rb.flags;
    P.glanes = glanes;
    ctx->last_ray_lanes = glanes;
    SCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    SCHK(af_launch_rays(&P, ctx->stream));
    SCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    std::vector<double> t(2 * m);
    std::vector<int> l(2 * m), fl(2 * m);
    SCHK(hipMemcpyAsync(t.data(), rb.t, 8 * (size_t)(2 * m), hipMemcpyDeviceToHost, ctx->stream));
    SCHK(hipMemcpyAsync(l.data(), rb.len, 4 * (size_t)(2 * m), hipMemcpyDeviceToHost, ctx->stream));
    SCHK(hipMemcpyAsync(fl.data(), rb.flags, 4 * (size_t)(2 * m), hipMemcpyDeviceToHost, ctx->stream));
    SCHK(hipStreamSynchronize(ctx->stream));
    {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]);
      ctx->t_ray_kernel += ms;
    }
    std::vector<long long> off(m + 1, 0);
    for (int p = 0; p < m; p++) {
      const int k = live[p];
      // a leg has at least its two end points and at most max_pts (find_ray_kernel's capacity)
      if (l[2 * p] < 2 || l[2 * p + 1] < 2 || l[2 * p] > max_pts || l[2 * p + 1] > max_pts) {
        dfree(d_packed);
        release_kept_rays(ctx);
        return fail(ctx, ALIFMM_E_KERNEL, "skip_rays: pair %d has legs of %d and %d points", k, l[2 * p], l[2 * p + 1]);
      }
      lens[k] = l[2 * p] + l[2 * p + 1] - 1;
      flg[k] = fl[2 * p] | fl[2 * p + 1];
      tms[k] = (flg[k] & 6) ? 0.0 : t[2 * p] + t[2 * p + 1];
      off[p + 1] = off[p] + lens[k];
    }
    if (!(ray_xy || keep)) continue;
    dfree(d_packed);
    d_packed = nullptr;
    SCHK(dalloc(&d_packed, (size_t)2 * off[m]));
    SCHK(hipMemcpyAsync(rb.off, off.data(), 8 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    SCHK(hipEventRecord(ctx->ev[2], ctx->stream));
    SCHK(af_launch_skip_join(rb.rx, rb.ry, rb.len, rb.off, m, max_pts, d_packed, ctx->stream));
    SCHK(hipEventRecord(ctx->ev[3], ctx->stream));
    SCHK(hipEventSynchronize(ctx->ev[3]));
    {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]);
      ctx->t_skip_join += ms;
    }
    if (dev_keep && kept_bytes + 16 * (size_t)off[m] > keep_budget) {
      dev_keep = false;
      SCHK(spill_kept_rays(ctx, ids.data(), lens, staged));
    }
    if (dev_keep) {  // the chunk's joined rays stay on the device (the context owns them now)
      kept_bytes += 16 * (size_t)off[m];
      ctx->kept_dev.push_back({d_packed, (int64_t)off[m]});
      ctx->kept_pts += off[m];
      d_packed = nullptr;
      continue;
    }
    if (staged.empty()) staged.assign(npairs, {});
    std::vector<double> packed(2 * (size_t)off[m]);
    SCHK(hipMemcpyAsync(packed.data(), d_packed, 16 * (size_t)off[m], hipMemcpyDeviceToHost, ctx->stream));
    SCHK(hipStreamSynchronize(ctx->stream));
    for (int p = 0; p < m; p++) staged[live[p]].assign(packed.begin() + 2 * off[p], packed.begin() + 2 * off[p + 1]);
  }
#undef SCHK
  dfree(d_packed);
  int64_t total = 0;
  for (int k = 0; k < npairs; k++) total += lens[k];
  int rc = ALIFMM_OK;
  if (ray_xy && total > ray_xy_cap)
    rc = fail(ctx, ALIFMM_E_ARG, "skip_rays: ray_xy capacity %lld < %lld", (long long)ray_xy_cap, (long long)total);
  if (!rc) {
    int64_t o = 0;
    for (int k = 0; k < npairs; k++) {
      if (pick_time) pick_time[k] = R.pick[k];
      if (hit) hit[k] = R.hit[k];
      times[k] = tms[k];
      ray_len[k] = lens[k];
      if (flags) flags[k] = flg[k];
      if (ray_xy) std::copy(staged[k].begin(), staged[k].end(), ray_xy + 2 * o);
      o += lens[k];
    }
    if (keep && !dev_keep) {
      if (staged.empty()) staged.assign(npairs, {});
      ctx->kept_rays.swap(staged);
      ctx->kept_pts = total;
    }
  }
  if (rc || (dev_keep && ctx->kept_pts != total)) {
    release_kept_rays(ctx);
    if (!rc) rc = fail(ctx, ALIFMM_E_KERNEL, "skip_rays: kept points do not add up to the ray lengths");
  }
  ctx->t_find_rays = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
  if (rb.pts * 2 * sizeof(double) > kRayBufKeepBytes) free_ray_bufs(ctx);
  return rc;
}

int alifmm_put_field(alifmm_ctx* ctx, int slot, int subgrid, const double* data) {
  if (!ctx || !ctx->have_model || slot < 0 || !data) return fail(ctx, ALIFMM_E_ARG, "put_field: bad args");
  int fz, fx;
  int rc = alifmm_field_shape(ctx, subgrid, &fz, &fx);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  if ((rc = af_ensure_field(ctx, slot, subgrid, fz, fx))) return rc;
  HIPCHK(hipMemcpy(ctx->fields[slot].d, data, (size_t)fz * fx * 8, hipMemcpyHostToDevice));
  return ALIFMM_OK;
}

// The argument checks of alifmm_tfm, shared with alifmm_tfm_f64 and alifmm_tfm_lsq (`what` names the
// caller in messages); on success tab = the transmitters' fields, then the receivers', fx = their
// row pitch
static int tfm_check(alifmm_ctx* ctx, const char* what, int subgrid, int ntx, const int32_t* tx_slot, int nrx,
                     const int32_t* rx_slot, const void* fmc, int nt, int ncomp, double t0, double fs, int iz0, int ix0,
                     int niz, int nix, int step, const void* image, std::vector<const double*>& tab, int* fx_out) {
  if (!ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "%s: no model", what);
  if (!tx_slot || !rx_slot || !fmc || !image) return fail(ctx, ALIFMM_E_ARG, "%s: null pointer", what);
  if (ntx < 1 || nrx < 1 || nt < 2) return fail(ctx, ALIFMM_E_ARG, "%s: ntx %d, nrx %d, nt %d", what, ntx, nrx, nt);
  if (ncomp != 1 && ncomp != 2) return fail(ctx, ALIFMM_E_ARG, "%s: ncomp %d is not 1 or 2", what, ncomp);
  if (!(std::isfinite(fs) && fs > 0) || !std::isfinite(t0)) return fail(ctx, ALIFMM_E_ARG, "%s: fs %g, t0 %g", what, fs, t0);
  if (step < 1 || niz < 1 || nix < 1) return fail(ctx, ALIFMM_E_ARG, "%s: step %d, window %d x %d", what, step, niz, nix);
  // the slots: resident fields of `subgrid`, one shape
  int fz = 0, fx = 0;
  tab.assign((size_t)ntx + nrx, nullptr);
  for (int k = 0; k < ntx + nrx; k++) {
    const int s = k < ntx ? tx_slot[k] : rx_slot[k - ntx];
    if (s < 0 || s >= (int)ctx->fields.size() || !ctx->fields[s].d)
      return fail(ctx, ALIFMM_E_ARG, "%s: no field in slot %d", what, s);
    const Field& f = ctx->fields[s];
    if (f.sg != subgrid) return fail(ctx, ALIFMM_E_ARG, "%s: slot %d holds a subgrid-%d field, not %d", what, s, f.sg, subgrid);
    if (k == 0) fz = f.nz, fx = f.nx;
    if (f.nz != fz || f.nx != fx)
      return fail(ctx, ALIFMM_E_ARG, "%s: slot %d is %d x %d, slot %d is %d x %d", what, s, f.nz, f.nx, tx_slot[0], fz, fx);
    tab[k] = f.d;
  }
  if (iz0 < 0 || ix0 < 0 || (int64_t)iz0 + (int64_t)step * (niz - 1) > fz - 1 ||
      (int64_t)ix0 + (int64_t)step * (nix - 1) > fx - 1)
    return fail(ctx, ALIFMM_E_ARG, "%s: window (%d, %d) + %d x (%d, %d) outside the %d x %d field", what, iz0, ix0, step,
                niz, nix, fz, fx);
  *fx_out = fx;
  return ALIFMM_OK;
}

// What alifmm_tfm, alifmm_tfm_f64 and alifmm_tfm_coh share after the checks: the data, the weights
// and the slot table `tab` go into the context's grow-only buffers (their copies' host time into
// *t_upload), the image's buffer holds nimg values, and P is filled in full
static int tfm_stage(alifmm_ctx* ctx, bool f64, const std::vector<const double*>& tab, int fx, int ntx, int nrx,
                     const void* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w, int iz0, int ix0,
                     int niz, int nix, int step, af::TfmParams* Pout, double* t_upload) {
  const size_t npair = (size_t)ntx * nrx, ndata = npair * (size_t)nt * ncomp, nimg = (size_t)niz * nix * ncomp;
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::TfmBufs& B = ctx->tfm;
  void* dfmc = nullptr;
  if (f64) {
    HIPCHK(dgrow(&B.fmc64, &B.fmc64_n, ndata));
    dfmc = B.fmc64;
  } else {
    HIPCHK(dgrow(&B.fmc, &B.fmc_n, ndata));
    dfmc = B.fmc;
  }
  if (pair_w) HIPCHK(dgrow(&B.w, &B.w_n, npair));
  HIPCHK(dgrow(&B.tab, &B.tab_n, tab.size()));
  HIPCHK(dgrow(&B.img, &B.img_n, nimg));
  const auto c0 = std::chrono::steady_clock::now();
  HIPCHK(hipMemcpy(dfmc, fmc, ndata * (f64 ? sizeof(double) : sizeof(float)), hipMemcpyHostToDevice));
  if (pair_w) HIPCHK(hipMemcpy(B.w, pair_w, npair * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(B.tab, tab.data(), tab.size() * sizeof(double*), hipMemcpyHostToDevice));
  *t_upload = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
  af::TfmParams& P = *Pout;
  P.tx = B.tab;
  P.rx = B.tab + ntx;
  P.fmc = f64 ? nullptr : B.fmc;
  P.fmc64 = f64 ? B.fmc64 : nullptr;
  P.pair_w = pair_w ? B.w : nullptr;
  P.image = B.img;
  P.t0 = t0;
  P.fs = fs;
  P.ntx = ntx;
  P.nrx = nrx;
  P.nt = nt;
  P.ncomp = ncomp;
  P.fnx = fx;
  P.iz0 = iz0;
  P.ix0 = ix0;
  P.niz = niz;
  P.nix = nix;
  P.step = step;
  return ALIFMM_OK;
}

// `launch(stream)` between the context's two events, waited for; its device time into *t_kernel
extern "C++" template <class F>
static int tfm_timed(alifmm_ctx* ctx, F launch, double* t_kernel) {
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  HIPCHK(launch(ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
  *t_kernel = ms;
  return ALIFMM_OK;
}

// alifmm_tfm (fmc float32) and alifmm_tfm_f64 (f64: fmc float64): the same call but for the data's type
static int tfm_impl(alifmm_ctx* ctx, const char* what, bool f64, int subgrid, int ntx, const int32_t* tx_slot, int nrx,
                    const int32_t* rx_slot, const void* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w,
                    int iz0, int ix0, int niz, int nix, int step, double* image) {
  if (!ctx) return ALIFMM_E_ARG;
  std::vector<const double*> tab;
  int fx = 0;
  if (int rc = tfm_check(ctx, what, subgrid, ntx, tx_slot, nrx, rx_slot, fmc, nt, ncomp, t0, fs, iz0, ix0, niz, nix, step,
                         image, tab, &fx))
    return rc;
  af::TfmParams P;
  if (int rc = tfm_stage(ctx, f64, tab, fx, ntx, nrx, fmc, nt, ncomp, t0, fs, pair_w, iz0, ix0, niz, nix, step, &P,
                         &ctx->t_tfm_upload))
    return rc;
  const int chunk = ctx->tfm_chunk;
  const auto launch = [&](hipStream_t st) { return f64 ? af_launch_tfm_f64(&P, chunk, st) : af_launch_tfm(&P, chunk, st); };
  if (int rc = tfm_timed(ctx, launch, &ctx->t_tfm_kernel)) return rc;
  HIPCHK(hipMemcpy(image, P.image, (size_t)niz * nix * ncomp * sizeof(double), hipMemcpyDeviceToHost));
  return ALIFMM_OK;
}

int alifmm_tfm(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx, const int32_t* rx_slot,
               const float* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w, int iz0, int ix0,
               int niz, int nix, int step, double* image) {
  return tfm_impl(ctx, "tfm", false, subgrid, ntx, tx_slot, nrx, rx_slot, fmc, nt, ncomp, t0, fs, pair_w, iz0, ix0, niz,
                  nix, step, image);
}

int alifmm_tfm_f64(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx, const int32_t* rx_slot,
                   const double* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w, int iz0, int ix0,
                   int niz, int nix, int step, double* image) {
  return tfm_impl(ctx, "tfm_f64", true, subgrid, ntx, tx_slot, nrx, rx_slot, fmc, nt, ncomp, t0, fs, pair_w, iz0, ix0, niz,
                  nix, step, image);
}

int alifmm_tfm_coh(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx, const int32_t* rx_slot,
                   const float* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w, int iz0, int ix0,
                   int niz, int nix, int step, int kind, double* image, double* factor, double* sums) {
  if (!ctx) return ALIFMM_E_ARG;
  std::vector<const double*> tab;
  int fx = 0;
  if (int rc = tfm_check(ctx, "tfm_coh", subgrid, ntx, tx_slot, nrx, rx_slot, fmc, nt, ncomp, t0, fs, iz0, ix0, niz, nix,
                         step, image, tab, &fx))
    return rc;
  if (!factor) return fail(ctx, ALIFMM_E_ARG, "tfm_coh: null pointer");
  if (kind < 1 || kind > 3) return fail(ctx, ALIFMM_E_ARG, "tfm_coh: kind %d is not 1 (CF), 2 (SCF) or 3 (PCF)", kind);
  if (kind == 3 && ncomp != 2) return fail(ctx, ALIFMM_E_ARG, "tfm_coh: kind 3 (PCF) needs ncomp 2, not %d", ncomp);
  af::TfmCohParams Q;
  if (int rc = tfm_stage(ctx, false, tab, fx, ntx, nrx, fmc, nt, ncomp, t0, fs, pair_w, iz0, ix0, niz, nix, step, &Q.T,
                         &ctx->t_tfm_coh_upload))
    return rc;
  const size_t npix = (size_t)niz * nix;
  alifmm_ctx::TfmBufs& B = ctx->tfm;
  HIPCHK(dgrow(&B.coh_f, &B.coh_f_n, npix));
  if (sums) HIPCHK(dgrow(&B.coh_s, &B.coh_s_n, 3 * npix));
  Q.factor = B.coh_f;
  Q.sums = sums ? B.coh_s : nullptr;
  const int chunk = ctx->tfm_chunk;
  const auto launch = [&](hipStream_t st) { return af_launch_tfm_coh(&Q, kind, chunk, st); };
  if (int rc = tfm_timed(ctx, launch, &ctx->t_tfm_coh_kernel)) return rc;
  HIPCHK(hipMemcpy(image, Q.T.image, npix * ncomp * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(factor, Q.factor, npix * sizeof(double), hipMemcpyDeviceToHost));
  if (sums) HIPCHK(hipMemcpy(sums, Q.sums, 3 * npix * sizeof(double), hipMemcpyDeviceToHost));
  return ALIFMM_OK;
}

int alifmm_tfm_model(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx, const int32_t* rx_slot,
                     const double* refl, int ncomp, int nt, double t0, double fs, const float* pair_w, int iz0, int ix0,
                     int niz, int nix, int step, double* fmc_out) {
  if (!ctx) return ALIFMM_E_ARG;
  if (!ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "tfm_model: no model");
  if (!tx_slot || !rx_slot || !refl || !fmc_out) return fail(ctx, ALIFMM_E_ARG, "tfm_model: null pointer");
  if (ntx < 1 || nrx < 1 || nt < 2) return fail(ctx, ALIFMM_E_ARG, "tfm_model: ntx %d, nrx %d, nt %d", ntx, nrx, nt);
  if (ncomp != 1 && ncomp != 2) return fail(ctx, ALIFMM_E_ARG, "tfm_model: ncomp %d is not 1 or 2", ncomp);
  if (!(std::isfinite(fs) && fs > 0) || !std::isfinite(t0)) return fail(ctx, ALIFMM_E_ARG, "tfm_model: fs %g, t0 %g", fs, t0);
  if (step < 1 || niz < 1 || nix < 1) return fail(ctx, ALIFMM_E_ARG, "tfm_model: step %d, window %d x %d", step, niz, nix);
  // the slots: resident fields of `subgrid`, one shape (as alifmm_tfm)
  int fz = 0, fx = 0;
  std::vector<const double*> tab((size_t)ntx + nrx);
  for (int k = 0; k < ntx + nrx; k++) {
    const int s = k < ntx ? tx_slot[k] : rx_slot[k - ntx];
    if (s < 0 || s >= (int)ctx->fields.size() || !ctx->fields[s].d)
      return fail(ctx, ALIFMM_E_ARG, "tfm_model: no field in slot %d", s);
    const Field& f = ctx->fields[s];
    if (f.sg != subgrid)
      return fail(ctx, ALIFMM_E_ARG, "tfm_model: slot %d holds a subgrid-%d field, not %d", s, f.sg, subgrid);
    if (k == 0) fz = f.nz, fx = f.nx;
    if (f.nz != fz || f.nx != fx)
      return fail(ctx, ALIFMM_E_ARG, "tfm_model: slot %d is %d x %d, slot %d is %d x %d", s, f.nz, f.nx, tx_slot[0], fz, fx);
    tab[k] = f.d;
  }
  if (iz0 < 0 || ix0 < 0 || (int64_t)iz0 + (int64_t)step * (niz - 1) > fz - 1 ||
      (int64_t)ix0 + (int64_t)step * (nix - 1) > fx - 1)
    return fail(ctx, ALIFMM_E_ARG, "tfm_model: window (%d, %d) + %d x (%d, %d) outside the %d x %d field", iz0, ix0, step,
                niz, nix, fz, fx);
  const int rg = ctx->tfm_model_rx;
  const int64_t ngroups = (int64_t)ntx * ((nrx + rg - 1) / rg);
  if (ngroups > 0x7fffffffLL)
    return fail(ctx, ALIFMM_E_ARG, "tfm_model: %d x %d pairs are more than one launch takes", ntx, nrx);
  // the map: every value finite; the pixels that are not all zero, in raster order, as field offsets
  // (a zero pixel never reaches the device)
  const auto c0 = std::chrono::steady_clock::now();
  std::vector<int64_t> pix;
  std::vector<double> val;
  for (int i = 0; i < niz; i++)
    for (int j = 0; j < nix; j++) {
      const double* x = refl + ((int64_t)i * nix + j) * ncomp;
      bool any = false;
      for (int c = 0; c < ncomp; c++) {
        if (!std::isfinite(x[c]))
          return fail(ctx, ALIFMM_E_ARG, "tfm_model: refl[%d][%d][%d] is %g", i, j, c, x[c]);
        any |= x[c] != 0.0;
      }
      if (!any) continue;
      pix.push_back(af::tfm_model_pixel_offset(iz0, ix0, step, fx, i, j));
      for (int c = 0; c < ncomp; c++) val.push_back(x[c]);
    }
  const size_t npix = pix.size(), npair = (size_t)ntx * nrx, nout = npair * (size_t)nt * ncomp;
  // the knobs in force
  const int tile = af::tfm_model_tile(ctx->tfm_model_tile, nt, ncomp, rg);
  int64_t slabs = ctx->tfm_model_slabs;
  if (slabs == 0) {  // two workgroups per CU where the pairs alone do not give them, a slab no shorter than a workgroup
    slabs = (2 * (int64_t)std::max(ctx->n_cu, 1) + ngroups - 1) / ngroups;
    slabs = std::min<int64_t>(slabs, ((int64_t)npix + 1023) / 1024);
  }
  slabs = std::max<int64_t>(1, std::min<int64_t>({slabs, 64, (int64_t)npix}));
  ctx->tfm_model_tile_used = tile;
  ctx->tfm_model_slabs_used = (int)slabs;
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::TfmModelBufs& B = ctx->tfm_model;
  HIPCHK(dgrow(&B.pix, &B.pix_n, npix));
  HIPCHK(dgrow(&B.refl, &B.refl_n, val.size()));
  if (pair_w) HIPCHK(dgrow(&B.w, &B.w_n, npair));
  HIPCHK(dgrow(&B.tab, &B.tab_n, tab.size()));
  HIPCHK(dgrow(&B.out, &B.out_n, nout));
  if (npix) {
    HIPCHK(hipMemcpy(B.pix, pix.data(), npix * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(B.refl, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (pair_w) HIPCHK(hipMemcpy(B.w, pair_w, npair * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(B.tab, tab.data(), tab.size() * sizeof(double*), hipMemcpyHostToDevice));
  ctx->t_tfm_model_upload = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
  af::TfmModelParams P;
  P.tx = B.tab;
  P.rx = B.tab + ntx;
  P.pix = B.pix;
  P.refl = B.refl;
  P.pair_w = pair_w ? B.w : nullptr;
  P.out = B.out;
  P.t0 = t0;
  P.fs = fs;
  P.npix = (int64_t)npix;
  P.ntx = ntx;
  P.nrx = nrx;
  P.nt = nt;
  P.ncomp = ncomp;
  P.rg = rg;
  P.tile = tile;
  P.slabs = (int)slabs;
  P.combine = ctx->tfm_model_combine;
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  // one slab stores every sample of its traces; several add into zeros; no pixel: all zeros
  if (slabs > 1 || npix == 0) HIPCHK(hipMemsetAsync(B.out, 0, nout * sizeof(double), ctx->stream));
  if (npix) HIPCHK(af_launch_tfm_model(&P, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
  ctx->t_tfm_model_kernel = ms;
  HIPCHK(hipMemcpy(fmc_out, B.out, nout * sizeof(double), hipMemcpyDeviceToHost));
  return ALIFMM_OK;
}

// The device half of alifmm_tfm_lsq, after the checks: hipSuccess or the first error (the caller
// frees the call's buffers on one).  out: iterations, reason, |d|², gamma_0, gamma, |r|²
static hipError_t tfm_lsq_run(alifmm_ctx* ctx, const std::vector<const double*>& tab, int fx, int ntx, int nrx,
                              const double* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w, int iz0,
                              int ix0, int niz, int nix, int step, double damp, double smooth, int max_iter, double tol,
                              double* image, double* resid, double* out6) {
#define LSQ(call)                          \
  do {                                     \
    hipError_t e_ = (call);                \
    if (e_ != hipSuccess) return e_;       \
  } while (0)
  const size_t npix = (size_t)niz * nix, npair = (size_t)ntx * nrx;
  const size_t nd = npair * (size_t)nt * ncomp, ni = npix * ncomp;
  const int rg = ctx->tfm_model_rx;
  const int64_t ngroups = (int64_t)ntx * ((nrx + rg - 1) / rg);
  // the modelling kernel's knobs in force (alifmm_tfm_model), every pixel of the window counting
  const int tile = af::tfm_model_tile(ctx->tfm_model_tile, nt, ncomp, rg);
  int64_t slabs = ctx->tfm_model_slabs;
  if (slabs == 0) {
    slabs = (2 * (int64_t)std::max(ctx->n_cu, 1) + ngroups - 1) / ngroups;
    slabs = std::min<int64_t>(slabs, ((int64_t)npix + 1023) / 1024);
  }
  slabs = std::max<int64_t>(1, std::min<int64_t>({slabs, 64, (int64_t)npix}));
  ctx->tfm_model_tile_used = tile;
  ctx->tfm_model_slabs_used = (int)slabs;
  LSQ(hipSetDevice(ctx->device));
  alifmm_ctx::TfmLsqBufs& B = ctx->tfm_lsq;
  LSQ(dgrow(&B.data, &B.data_n, 2 * nd));
  LSQ(dgrow(&B.img, &B.img_n, 4 * ni));
  LSQ(dgrow(&B.small, &B.small_n, (size_t)af::kSolveMaxParts + af::kSolScalars));
  LSQ(dgrow(&B.pix, &B.pix_n, npix));
  if (pair_w) LSQ(dgrow(&B.w, &B.w_n, npair));
  LSQ(dgrow(&B.tab, &B.tab_n, tab.size()));
  af::SolveVecs V;
  V.x = B.img;
  V.p = B.img + ni;
  V.s = B.img + 2 * ni;
  V.t = B.img + 3 * ni;
  V.xs = nullptr;
  V.r = B.data;
  V.q = B.data + nd;
  V.parts = B.small;
  V.scal = B.small + af::kSolveMaxParts;
  V.damp2 = damp * damp;
  V.smooth2 = smooth * smooth;
  const auto c0 = std::chrono::steady_clock::now();
  LSQ(hipMemcpy(V.r, fmc, nd * sizeof(double), hipMemcpyHostToDevice));
  if (pair_w) LSQ(hipMemcpy(B.w, pair_w, npair * sizeof(float), hipMemcpyHostToDevice));
  LSQ(hipMemcpy(B.tab, tab.data(), tab.size() * sizeof(double*), hipMemcpyHostToDevice));
  ctx->t_tfm_lsq_upload = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
  af::TfmLsqDims G;
  G.niz = niz;
  G.nix = nix;
  G.nc = ncomp;
  G.nimg = (int64_t)ni;
  G.ndata = (int64_t)nd;
  af::TfmParams T;  // t = Aᵀ r
  T.tx = B.tab;
  T.rx = B.tab + ntx;
  T.fmc = nullptr;
  T.fmc64 = V.r;
  T.pair_w = pair_w ? B.w : nullptr;
  T.image = V.t;
  T.t0 = t0;
  T.fs = fs;
  T.ntx = ntx;
  T.nrx = nrx;
  T.nt = nt;
  T.ncomp = ncomp;
  T.fnx = fx;
  T.iz0 = iz0;
  T.ix0 = ix0;
  T.niz = niz;
  T.nix = nix;
  T.step = step;
  af::TfmModelParams M;  // q = A p
  M.tx = B.tab;
  M.rx = B.tab + ntx;
  M.pix = B.pix;
  M.refl = V.p;
  M.pair_w = pair_w ? B.w : nullptr;
  M.out = V.q;
  M.t0 = t0;
  M.fs = fs;
  M.npix = (int64_t)npix;
  M.ntx = ntx;
  M.nrx = nrx;
  M.nt = nt;
  M.ncomp = ncomp;
  M.rg = rg;
  M.tile = tile;
  M.slabs = (int)slabs;
  M.combine = ctx->tfm_model_combine;
  hipStream_t st = ctx->stream;
  // one scalar of the device's (8 bytes) after the work queued so far
  auto scalar = [&](int which, double* v) {
    hipError_t e = hipMemcpyAsync(v, V.scal + which, 8, hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
  };
  LSQ(hipEventRecord(ctx->ev[0], st));
  LSQ(af_launch_tfm_lsq_pix(iz0, ix0, step, fx, niz, nix, B.pix, st));
  LSQ(hipMemsetAsync(V.x, 0, 2 * ni * sizeof(double), st));  // x = p = 0
  LSQ(hipMemsetAsync(V.scal, 0, af::kSolScalars * sizeof(double), st));
  double rhs2 = 0, gamma0 = 0, gamma = 0, res2 = 0;
  LSQ(af_launch_solve_norm(V.r, (long)nd, &V, st));
  LSQ(scalar(af::kSolNorm, &rhs2));
  // x = 0: s = Aᵀ d, p = s, gamma_0 = |s|²
  LSQ(af_launch_tfm_f64(&T, ctx->tfm_chunk, st));
  LSQ(af_launch_tfm_lsq_grad(&G, &V, 1, st));
  LSQ(scalar(af::kSolReport, &gamma0));
  gamma = gamma0;
  int iters = 0, reason = 1;
  if (gamma0 == 0.0) reason = 2;
  else
    for (int it = 1; it <= max_iter; it++) {
      // several slabs add into q with atomics: zeroed every iteration
      if (slabs > 1) LSQ(hipMemsetAsync(V.q, 0, nd * sizeof(double), st));
      LSQ(af_launch_tfm_model(&M, st));
      LSQ(af_launch_tfm_lsq_step(&G, &V, st));
      LSQ(af_launch_tfm_f64(&T, ctx->tfm_chunk, st));
      LSQ(af_launch_tfm_lsq_grad(&G, &V, 0, st));
      double rep = 0;
      LSQ(scalar(af::kSolReport, &rep));  // the one read of an iteration: the new gamma, -1: qq was 0
      if (rep < 0) {
        reason = 2;
        break;
      }
      gamma = rep;
      iters = it;
      if (gamma <= tol * tol * gamma0) {
        reason = 0;
        break;
      }
    }
  LSQ(af_launch_solve_norm(V.r, (long)nd, &V, st));
  LSQ(scalar(af::kSolNorm, &res2));
  LSQ(hipEventRecord(ctx->ev[1], st));
  LSQ(hipStreamSynchronize(st));
  float ms = 0;
  LSQ(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
  ctx->t_tfm_lsq_kernel = ms;
  ctx->tfm_lsq_iters = iters;
  LSQ(hipMemcpy(image, V.x, ni * sizeof(double), hipMemcpyDeviceToHost));
  if (resid) LSQ(hipMemcpy(resid, V.r, nd * sizeof(double), hipMemcpyDeviceToHost));
  out6[0] = iters, out6[1] = reason, out6[2] = rhs2, out6[3] = gamma0, out6[4] = gamma, out6[5] = res2;
  return hipSuccess;
#undef LSQ
}

int alifmm_tfm_lsq(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx, const int32_t* rx_slot,
                   const double* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w, int iz0, int ix0,
                   int niz, int nix, int step, double damp, double smooth, int max_iter, double tol, double* image,
                   double* resid, double* info8) {
  if (!ctx) return ALIFMM_E_ARG;
  std::vector<const double*> tab;
  int fx = 0;
  if (int rc = tfm_check(ctx, "tfm_lsq", subgrid, ntx, tx_slot, nrx, rx_slot, fmc, nt, ncomp, t0, fs, iz0, ix0, niz, nix,
                         step, image, tab, &fx))
    return rc;
  if (!info8) return fail(ctx, ALIFMM_E_ARG, "tfm_lsq: info8 is NULL");
  if (!(damp >= 0) || !std::isfinite(damp)) return fail(ctx, ALIFMM_E_ARG, "tfm_lsq: damp %g", damp);
  if (!(smooth >= 0) || !std::isfinite(smooth)) return fail(ctx, ALIFMM_E_ARG, "tfm_lsq: smooth %g", smooth);
  if (max_iter < 1) return fail(ctx, ALIFMM_E_ARG, "tfm_lsq: max_iter %d", max_iter);
  if (!(tol >= 0) || !std::isfinite(tol)) return fail(ctx, ALIFMM_E_ARG, "tfm_lsq: tol %g", tol);
  const int rg = ctx->tfm_model_rx;
  if ((int64_t)ntx * ((nrx + rg - 1) / rg) > 0x7fffffffLL)
    return fail(ctx, ALIFMM_E_ARG, "tfm_lsq: %d x %d pairs are more than one launch takes", ntx, nrx);
  const size_t nd = (size_t)ntx * nrx * (size_t)nt * ncomp;
  for (size_t k = 0; k < nd; k++)
    if (!std::isfinite(fmc[k])) return fail(ctx, ALIFMM_E_ARG, "tfm_lsq: fmc[%zu] is not finite", k);
  double o[6];
  const hipError_t e = tfm_lsq_run(ctx, tab, fx, ntx, nrx, fmc, nt, ncomp, t0, fs, pair_w, iz0, ix0, niz, nix, step, damp,
                                   smooth, max_iter, tol, image, resid, o);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);
    free_tfm_lsq_bufs(ctx);
    return fail(ctx, ALIFMM_E_HIP, "tfm_lsq: %s", hipGetErrorString(e));
  }
  const double info[8] = {o[0], sqrt(o[3]), sqrt(o[4]), sqrt(o[2]), sqrt(o[5]), o[1], 0.0, 0.0};
  memcpy(info8, info, sizeof info);
  return ALIFMM_OK;
}

// The front half of a sensitivity request, shared by alifmm_ray_sens and alifmm_sens_op_build (`what`
// names the caller in messages): the rays' first points, the chunks of whole rays whose points are
// on the device together, the per-ray arrays uploaded, the count pass run, and the row offsets and
// status of every ray on the host.  run_chunk then runs the fill pass chunk by chunk.
struct SensRequest {
  struct Chunk {
    int r0, r1;       // [first ray, end ray)
    const double* d;  // device pointer (kept points) or null (host points, uploaded into the context's buffer)
  };
  const char* what = "";
  const double* ray_xy = nullptr;
  std::vector<long long> off, rows;
  std::vector<int32_t> status;
  std::vector<Chunk> chunks;
  af::SensParams P;
  int resident = -1;  // the host chunk whose points the context's buffer holds
  long long total = 0;
};

static int sens_check_args(alifmm_ctx* ctx, const char* what, int subgrid, int nrays, const int32_t* ray_len) {
  if (!ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "%s: no model", what);
  if (subgrid < 1) return fail(ctx, ALIFMM_E_ARG, "%s: subgrid %d", what, subgrid);
  if (nrays < 0) return fail(ctx, ALIFMM_E_ARG, "%s: nrays %d", what, nrays);
  if (!ray_len) return fail(ctx, ALIFMM_E_ARG, "%s: ray_len is NULL", what);
  return ALIFMM_OK;
}

// the chunk's points on the device, then one pass (count or fill) over its rays
static int sens_run_chunk(alifmm_ctx* ctx, SensRequest& R, int ci, bool fill) {
  alifmm_ctx::SensBufs& B = ctx->sens;
  af::SensParams& P = R.P;
  const SensRequest::Chunk& c = R.chunks[ci];
  const long long n = R.off[c.r1] - R.off[c.r0];
  if (c.d) {
    P.xy = c.d;
  } else {
    if (R.resident != ci) {
      HIPCHK(dgrow(&B.xy, &B.xy_n, (size_t)2 * std::max<long long>(n, 1)));
      const auto t0 = std::chrono::steady_clock::now();
      if (n) HIPCHK(hipMemcpy(B.xy, R.ray_xy + 2 * R.off[c.r0], (size_t)n * 16, hipMemcpyHostToDevice));
      ctx->t_sens_upload += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      R.resident = ci;
    }
    P.xy = B.xy;
  }
  P.pt0 = R.off[c.r0];
  P.ray0 = c.r0;
  P.nrays = c.r1 - c.r0;
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  HIPCHK(fill ? af_launch_sens_fill(&P, ctx->stream) : af_launch_sens_count(&P, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
  ctx->t_sens_kernel += ms;
  return ALIFMM_OK;
}

static int sens_count_pass(alifmm_ctx* ctx, SensRequest& R, int subgrid, int nrays, const int32_t* ray_len,
                           const int32_t* flags, const double* ray_xy, const double* ray_w) {
  const char* what = R.what;
  R.ray_xy = ray_xy;
  // the rays' first points; a length below 0 counts as no points
  std::vector<long long>& off = R.off;
  off.assign((size_t)nrays + 1, 0);
  for (int k = 0; k < nrays; k++) off[k + 1] = off[k] + std::max(ray_len[k], 0);
  const long long npts = off[nrays];
  std::vector<SensRequest::Chunk>& chunks = R.chunks;
  if (!ray_xy) {
    if (!ctx->kept_rays.empty())
      return fail(ctx, ALIFMM_E_ARG, "%s: the kept rays are staged on the host (several subgrids in one "
                                     "find_rays call); pass their points as ray_xy", what);
    if (npts != ctx->kept_pts)
      return fail(ctx, ALIFMM_E_ARG, "%s: ray_len adds up to %lld points, %lld are kept", what, npts,
                  (long long)ctx->kept_pts);
    int r = 0;
    for (auto& k : ctx->kept_dev) {
      const long long end = off[r] + k.npts;
      int r1 = r;
      while (r1 < nrays && off[r1 + 1] <= end) r1++;
      if (off[r1] != end) return fail(ctx, ALIFMM_E_ARG, "%s: ray_len does not match the kept rays", what);
      if (r1 > r) chunks.push_back({r, r1, k.d});
      r = r1;
    }
    if (r != nrays && off[r] != npts) return fail(ctx, ALIFMM_E_ARG, "%s: ray_len does not match the kept rays", what);
  } else {
    const long long kChunkPts = 1LL << 24;  // 256 MB of points per upload (a longer ray is a chunk of its own)
    for (int r = 0; r < nrays;) {
      int r1 = r + 1;
      while (r1 < nrays && off[r1 + 1] - off[r] <= kChunkPts) r1++;
      chunks.push_back({r, r1, nullptr});
      r = r1;
    }
  }
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::SensBufs& B = ctx->sens;
  const size_t nr = (size_t)nrays;
  ctx->t_sens_upload = ctx->t_sens_kernel = 0;
  ctx->sens_entries = 0;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms_since = [&](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(now() - t).count();
  };
  HIPCHK(dgrow(&B.off, &B.off_n, nr));
  HIPCHK(dgrow(&B.len, &B.len_n, nr));
  HIPCHK(dgrow(&B.cnt, &B.cnt_n, nr));
  HIPCHK(dgrow(&B.status, &B.status_n, nr));
  if (flags) HIPCHK(dgrow(&B.flags, &B.flags_n, nr));
  if (ray_w) HIPCHK(dgrow(&B.w, &B.w_n, nr));
  {
    const auto t0 = now();
    if (nrays) {
      HIPCHK(hipMemcpy(B.off, off.data(), nr * 8, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(B.len, ray_len, nr * 4, hipMemcpyHostToDevice));
      if (flags) HIPCHK(hipMemcpy(B.flags, flags, nr * 4, hipMemcpyHostToDevice));
      if (ray_w) HIPCHK(hipMemcpy(B.w, ray_w, nr * 8, hipMemcpyHostToDevice));
    }
    ctx->t_sens_upload += ms_since(t0);
  }
  af::SensParams& P = R.P;
  memset(&P, 0, sizeof P);
  P.M = dev_model(ctx);
  P.sg = subgrid;
  P.dnx = ctx->dnx;
  P.off = B.off;
  P.len = B.len;
  P.flags = flags ? B.flags : nullptr;
  P.w = ray_w ? B.w : nullptr;
  P.cnt = B.cnt;
  P.status = B.status;
  int rc = ALIFMM_OK;
  for (int ci = 0; ci < (int)chunks.size(); ci++)
    if ((rc = sens_run_chunk(ctx, R, ci, false))) return rc;
  // row offsets (rays outside every chunk have no points: no entries, status 0)
  R.rows.assign(nr + 1, 0);
  R.status.assign(nr, 0);
  {
    std::vector<long long> cnt(nr, 0);
    for (const SensRequest::Chunk& c : chunks) {
      HIPCHK(hipMemcpy(cnt.data() + c.r0, B.cnt + c.r0, (size_t)(c.r1 - c.r0) * 8, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(R.status.data() + c.r0, B.status + c.r0, (size_t)(c.r1 - c.r0) * 4, hipMemcpyDeviceToHost));
    }
    for (size_t k = 0; k < nr; k++) R.rows[k + 1] = R.rows[k] + cnt[k];
  }
  R.total = R.rows[nr];
  ctx->sens_entries = R.total;
  return ALIFMM_OK;
}

int alifmm_ray_sens(alifmm_ctx* ctx, int subgrid, int nrays, const int32_t* ray_len, const int32_t* flags,
                    const double* ray_xy, const double* ray_w, double* maps, int64_t* row_ptr, int64_t cap,
                    int32_t* col, double* len, double* time, double* dth, int32_t* ray_status) {
  if (!ctx) return ALIFMM_E_ARG;
  if (int rc = sens_check_args(ctx, "ray_sens", subgrid, nrays, ray_len)) return rc;
  const bool want_rows = col || len || time || dth;
  if (!maps && !row_ptr && !want_rows && !ray_status)
    return fail(ctx, ALIFMM_E_ARG, "ray_sens: nothing requested (maps, row_ptr and ray_status are NULL)");
  if (want_rows && !row_ptr) return fail(ctx, ALIFMM_E_ARG, "ray_sens: row arrays without row_ptr");
  SensRequest R;
  R.what = "ray_sens";
  int rc = sens_count_pass(ctx, R, subgrid, nrays, ray_len, flags, ray_xy, ray_w);
  if (rc) return rc;
  alifmm_ctx::SensBufs& B = ctx->sens;
  af::SensParams& P = R.P;
  const std::vector<long long>& rows = R.rows;
  const size_t nr = (size_t)nrays, ncell = (size_t)ctx->nz0 * ctx->nx0;
  const long long total = R.total;
  if (row_ptr)
    for (size_t k = 0; k <= nr; k++) row_ptr[k] = rows[k];
  if (ray_status && nrays) memcpy(ray_status, R.status.data(), nr * 4);
  if (want_rows && cap < total)
    return fail(ctx, ALIFMM_E_ARG, "ray_sens: cap %lld < %lld entries (row_ptr holds the sizes)", (long long)cap, total);
  if (!maps && !want_rows) return ALIFMM_OK;
  // the fill pass: maps in the context's buffer, rows in buffers of this call
  int32_t* d_col = nullptr;
  double* d_e[3] = {nullptr, nullptr, nullptr};
  auto cleanup = [&] {
    dfree(d_col);
    for (double* p : d_e) dfree(p);
  };
  double* const h_e[3] = {len, time, dth};
  hipError_t e = hipSuccess;
  if (maps) {
    e = dgrow(&B.maps, &B.maps_n, 3 * ncell);
    if (e == hipSuccess) e = hipMemsetAsync(B.maps, 0, 3 * ncell * 8, ctx->stream);
  }
  if (want_rows && total > 0) {
    if (e == hipSuccess) e = dgrow(&B.row, &B.row_n, nr);
    if (e == hipSuccess) e = hipMemcpy(B.row, rows.data(), nr * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && col) e = dalloc(&d_col, (size_t)total);
    for (int q = 0; q < 3; q++)
      if (e == hipSuccess && h_e[q]) e = dalloc(&d_e[q], (size_t)total);
  }
  if (e != hipSuccess) {
    cleanup();
    return fail(ctx, ALIFMM_E_HIP, "ray_sens: %s", hipGetErrorString(e));
  }
  P.maps = maps ? B.maps : nullptr;
  if (want_rows && total > 0) {
    P.row = B.row;
    P.col = d_col;
    P.elen = d_e[0];
    P.etime = d_e[1];
    P.edth = d_e[2];
  }
  if (total > 0 && (maps || P.row))
    for (int ci = 0; ci < (int)R.chunks.size() && !rc; ci++) rc = sens_run_chunk(ctx, R, ci, true);
  if (!rc && maps) {
    std::vector<D2HSeg> segs{{(const char*)B.maps, (char*)maps, 3 * ncell * 8}};
    rc = d2h_pageable(ctx, segs);
  }
  if (!rc && P.row) {
    std::vector<D2HSeg> segs;
    if (col) segs.push_back({(const char*)d_col, (char*)col, (size_t)total * 4});
    for (int q = 0; q < 3; q++)
      if (h_e[q]) segs.push_back({(const char*)d_e[q], (char*)h_e[q], (size_t)total * 8});
    rc = d2h_pageable(ctx, segs);
  }
  cleanup();
  return rc;
}

int alifmm_sens_op_release(alifmm_ctx* ctx) {
  if (!ctx) return ALIFMM_E_ARG;
  (void)hipSetDevice(ctx->device);
  sens_op_free(ctx);
  return ALIFMM_OK;
}

int alifmm_sens_op_build(alifmm_ctx* ctx, int subgrid, int nrays, const int32_t* ray_len, const int32_t* flags,
                         const double* ray_xy, int quantity, const double* col_scale, int64_t* entries,
                         int32_t* ray_status) {
  if (!ctx) return ALIFMM_E_ARG;
  if (int rc = sens_check_args(ctx, "sens_op_build", subgrid, nrays, ray_len)) return rc;
  if (quantity < 0 || quantity > 2) return fail(ctx, ALIFMM_E_ARG, "sens_op_build: quantity %d (0 len, 1 time, 2 dth)", quantity);
  const size_t nr = (size_t)nrays, ncell = (size_t)ctx->nz0 * ctx->nx0;
  if (col_scale)
    for (size_t c = 0; c < ncell; c++)
      if (!std::isfinite(col_scale[c])) return fail(ctx, ALIFMM_E_ARG, "sens_op_build: col_scale[%zu] is not finite", c);
  const auto t0 = std::chrono::steady_clock::now();
  SensRequest R;
  R.what = "sens_op_build";
  int rc = sens_count_pass(ctx, R, subgrid, nrays, ray_len, flags, ray_xy, nullptr);
  if (rc) return rc;
  sens_op_free(ctx);  // the request is good: the new operator replaces the resident one
  const long long total = R.total;
  if (entries) *entries = total;
  if (ray_status && nrays) memcpy(ray_status, R.status.data(), nr * 4);
  if (total >= (1LL << 31))
    return fail(ctx, ALIFMM_E_CAPACITY, "sens_op_build: %lld entries, an operator holds fewer than 2^31", total);
  alifmm_ctx::SensOpBufs& O = ctx->op;
  const size_t ne = (size_t)total;
  unsigned* scratch = nullptr;  // key | key2 | idx | idx2
  void* temp = nullptr;
  int* cursor = nullptr;
  const size_t temp_bytes = total ? af_solve_sort_temp(total, (long)ncell) : 0;
  auto drop = [&] {
    dfree(scratch);
    dfree(temp);
    dfree(cursor);
  };
  auto bail = [&](hipError_t e) {
    drop();
    sens_op_free(ctx);
    return fail(ctx, ALIFMM_E_HIP, "sens_op_build: %s", hipGetErrorString(e));
  };
  hipError_t e = dalloc(&O.row_ptr, nr + 1);
  if (e == hipSuccess) e = dalloc(&O.col, ne);
  if (e == hipSuccess) e = dalloc(&O.val, ne);
  if (e == hipSuccess) e = dalloc(&O.col_ptr, ncell + 1);
  if (e == hipSuccess) e = dalloc(&O.row, ne);
  if (e == hipSuccess) e = dalloc(&O.cval, ne);
  if (e == hipSuccess && col_scale) e = dalloc(&O.cs, ncell);
  if (e == hipSuccess) e = dalloc(&scratch, 4 * ne);
  if (e == hipSuccess) e = dalloc((char**)&temp, temp_bytes);
  if (e == hipSuccess) e = dalloc(&cursor, 3);
  if (e == hipSuccess) e = hipMemcpy(O.row_ptr, R.rows.data(), (nr + 1) * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess && col_scale) e = hipMemcpy(O.cs, col_scale, ncell * 8, hipMemcpyHostToDevice);
  if (e != hipSuccess) return bail(e);
  // the fill pass writes the CSR in place: the columns and the one quantity
  af::SensParams& P = R.P;
  P.row = O.row_ptr;
  P.col = O.col;
  (quantity == 0 ? P.elen : quantity == 1 ? P.etime : P.edth) = O.val;
  if (total > 0)
    for (int ci = 0; ci < (int)R.chunks.size() && !rc; ci++) rc = sens_run_chunk(ctx, R, ci, true);
  if (rc) {
    drop();
    sens_op_free(ctx);
    return rc;
  }
  af::SensOp& A = O.A;
  A.nrays = nrays;
  A.nz = ctx->nz0;
  A.nx = ctx->nx0;
  A.ncell = (long)ncell;
  A.entries = total;
  A.row_ptr = O.row_ptr;
  A.col = O.col;
  A.val = O.val;
  A.col_ptr = O.col_ptr;
  A.row = O.row;
  A.cval = O.cval;
  A.cs = O.cs;
  // the transposed copy, then the non-empty columns by length class: counted, then listed
  e = af_launch_solve_transpose(&A, O.col_ptr, O.row, O.cval, scratch, scratch + ne, scratch + 2 * ne, scratch + 3 * ne,
                                temp, temp_bytes, ctx->stream);
  int n3[3] = {0, 0, 0};
  if (e == hipSuccess) e = hipMemsetAsync(cursor, 0, sizeof n3, ctx->stream);
  if (e == hipSuccess) e = af_launch_solve_classify(O.col_ptr, (long)ncell, nullptr, cursor, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(n3, cursor, sizeof n3, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = dalloc(&O.cols, (size_t)n3[0] + n3[1] + n3[2]);
  const int first3[3] = {0, n3[0], n3[0] + n3[1]};
  if (e == hipSuccess) e = hipMemcpyAsync(cursor, first3, sizeof first3, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = af_launch_solve_classify(O.col_ptr, (long)ncell, O.cols, cursor, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return bail(e);
  for (int q = 0; q < 3; q++) {
    A.cols[q] = O.cols + first3[q];
    A.ncols[q] = n3[q];
  }
  drop();
  O.have = true;
  ctx->t_solve_build = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return ALIFMM_OK;
}

int alifmm_sens_op_apply(alifmm_ctx* ctx, int transpose, const double* in, double* out) {
  if (!ctx) return ALIFMM_E_ARG;
  if (!ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "sens_op_apply: no model");
  if (!ctx->op.have) return fail(ctx, ALIFMM_E_ARG, "sens_op_apply: no resident operator (alifmm_sens_op_build)");
  if (!in || !out) return fail(ctx, ALIFMM_E_ARG, "sens_op_apply: %s is NULL", in ? "out" : "in");
  const af::SensOp& A = ctx->op.A;
  const size_t nc = (size_t)A.ncell, nr = (size_t)A.nrays;
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::SolveBufs& S = ctx->solve;
  HIPCHK(dgrow(&S.cell, &S.cell_n, 5 * nc));
  HIPCHK(dgrow(&S.ray, &S.ray_n, 2 * nr));
  double* din = transpose ? S.ray : S.cell;
  double* dout = transpose ? S.cell : S.ray;
  const size_t nin = transpose ? nr : nc, nout = transpose ? nc : nr;
  if (nin) HIPCHK(hipMemcpy(din, in, nin * 8, hipMemcpyHostToDevice));
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  HIPCHK(transpose ? af_launch_solve_colprod(&A, din, dout, ctx->stream)
                   : af_launch_solve_rowprod(&A, din, S.cell + nc, dout, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
  ctx->t_solve_kernel = ms;
  if (nout) HIPCHK(hipMemcpy(out, dout, nout * 8, hipMemcpyDeviceToHost));
  return ALIFMM_OK;
}

int alifmm_sens_op_solve(alifmm_ctx* ctx, const double* rhs, double damp, double smooth, int max_iter, double tol,
                         double* x, double* info8) {
  if (!ctx) return ALIFMM_E_ARG;
  if (!ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "sens_op_solve: no model");
  if (!ctx->op.have) return fail(ctx, ALIFMM_E_ARG, "sens_op_solve: no resident operator (alifmm_sens_op_build)");
  if (!rhs || !x) return fail(ctx, ALIFMM_E_ARG, "sens_op_solve: %s is NULL", rhs ? "x" : "rhs");
  if (!(damp >= 0) || !std::isfinite(damp)) return fail(ctx, ALIFMM_E_ARG, "sens_op_solve: damp %g", damp);
  if (!(smooth >= 0) || !std::isfinite(smooth)) return fail(ctx, ALIFMM_E_ARG, "sens_op_solve: smooth %g", smooth);
  if (max_iter < 1) return fail(ctx, ALIFMM_E_ARG, "sens_op_solve: max_iter %d", max_iter);
  if (!(tol >= 0) || !std::isfinite(tol)) return fail(ctx, ALIFMM_E_ARG, "sens_op_solve: tol %g", tol);
  const af::SensOp& A = ctx->op.A;
  const size_t nc = (size_t)A.ncell, nr = (size_t)A.nrays;
  for (size_t k = 0; k < nr; k++)
    if (!std::isfinite(rhs[k])) return fail(ctx, ALIFMM_E_ARG, "sens_op_solve: rhs[%zu] is not finite", k);
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::SolveBufs& S = ctx->solve;
  HIPCHK(dgrow(&S.cell, &S.cell_n, 5 * nc));
  HIPCHK(dgrow(&S.ray, &S.ray_n, 2 * nr));
  HIPCHK(dgrow(&S.small, &S.small_n, (size_t)af::kSolveMaxParts + af::kSolScalars));
  af::SolveVecs V;
  V.x = S.cell;
  V.p = S.cell + nc;
  V.s = S.cell + 2 * nc;
  V.t = S.cell + 3 * nc;
  V.xs = S.cell + 4 * nc;
  V.r = S.ray;
  V.q = S.ray + nr;
  V.parts = S.small;
  V.scal = S.small + af::kSolveMaxParts;
  V.damp2 = damp * damp;
  V.smooth2 = smooth * smooth;
  hipStream_t st = ctx->stream;
  // one scalar of the device's (8 bytes) after the work queued so far
  auto scalar = [&](int which, double* v) {
    hipError_t e = hipMemcpyAsync(v, V.scal + which, 8, hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
  };
  if (nr) HIPCHK(hipMemcpy(V.r, rhs, nr * 8, hipMemcpyHostToDevice));
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  HIPCHK(hipMemsetAsync(V.x, 0, 2 * nc * 8, st));  // x = p = 0
  HIPCHK(hipMemsetAsync(V.scal, 0, af::kSolScalars * 8, st));
  double rhs2 = 0, gamma0 = 0, gamma = 0, res2 = 0;
  HIPCHK(af_launch_solve_norm(V.r, (long)nr, &V, st));
  HIPCHK(scalar(af::kSolNorm, &rhs2));
  // x = 0: s = Aᵀ rhs, p = s, gamma_0 = |s|²
  HIPCHK(af_launch_solve_colprod(&A, V.r, V.t, st));
  HIPCHK(af_launch_solve_start(&A, &V, st));
  HIPCHK(scalar(af::kSolReport, &gamma0));
  gamma = gamma0;
  int iters = 0, reason = 1;
  if (gamma0 == 0.0) reason = 2;
  else
    for (int it = 1; it <= max_iter; it++) {
      HIPCHK(af_launch_solve_iter(&A, &V, st));
      double rep = 0;
      HIPCHK(scalar(af::kSolReport, &rep));  // the one read of an iteration: the new gamma, -1: |q|² was 0
      if (rep < 0) {
        reason = 2;
        break;
      }
      gamma = rep;
      iters = it;
      if (gamma <= tol * tol * gamma0) {
        reason = 0;
        break;
      }
    }
  HIPCHK(af_launch_solve_norm(V.r, (long)nr, &V, st));
  HIPCHK(scalar(af::kSolNorm, &res2));
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
  ctx->t_solve_kernel = ms;
  ctx->solve_iters = iters;
  if (nc) HIPCHK(hipMemcpy(x, V.x, nc * 8, hipMemcpyDeviceToHost));
  if (info8) {
    const double info[8] = {(double)iters, sqrt(gamma0), sqrt(gamma), sqrt(rhs2), sqrt(res2), (double)reason,
                            (double)A.entries, 0.0};
    memcpy(info8, info, sizeof info);
  }
  return ALIFMM_OK;
}

int alifmm_time_between_points(alifmm_ctx* ctx, int n, const double* x1, const double* x2, const double* y1,
                               const double* y2, int subgrid, double* out) {
  if (!ctx || !ctx->have_model || n < 0 || subgrid < 1) return fail(ctx, ALIFMM_E_ARG, "time_between_points: bad args");
  if (n == 0) return ALIFMM_OK;
  HIPCHK(hipSetDevice(ctx->device));
  double* d = nullptr;
  HIPCHK(dalloc(&d, (size_t)5 * n));
  hipError_t e = hipSuccess;
  const double* src[4] = {x1, x2, y1, y2};
  for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipMemcpy(d + (size_t)k * n, src[k], 8 * (size_t)n, hipMemcpyHostToDevice);
  af::DevModel M = dev_model(ctx);
  if (e == hipSuccess) e = af_launch_tbp(&M, n, d, d + n, d + 2 * n, d + 3 * n, ctx->dnx, subgrid, d + 4 * n, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d + 4 * (size_t)n, 8 * (size_t)n, hipMemcpyDeviceToHost);
  dfree(d);
  if (e != hipSuccess) return fail(ctx, ALIFMM_E_HIP, "time_between_points: %s", hipGetErrorString(e));
  return ALIFMM_OK;
}

int alifmm_local_ops(alifmm_ctx* ctx, int op, int n, int pz, int px, const double* ttn, const int32_t* nsts,
                     const int32_t* iz, const int32_t* ix, const double* dnx, const double* dnz, const int32_t* nnz_arg,
                     const int32_t* nnx_arg, const double* cell_veln, const int64_t* cell_velpn, const double* cell_vm,
                     const int64_t* cell_stif, const double* tab, int ncol, double* out) {
  if (!ctx || (op != 0 && op != 1) || n < 0 || pz < 1 || px < 1 || ncol < 1)
    return fail(ctx, ALIFMM_E_ARG, "local_ops: bad args");
  if (n == 0) return ALIFMM_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t pn = (size_t)pz * px;
  std::vector<int> vp(n);
  for (int k = 0; k < n; k++) vp[k] = (int)cell_velpn[k];
  std::vector<double> st;
  if (cell_stif) {
    st.resize((size_t)5 * n);
    for (size_t k = 0; k < st.size(); k++) st[k] = (double)cell_stif[k];
  }
  // one device block: [ttn | cveln | cvm | dnx | dnz | tab | stif | out] doubles, [nsts | iz | ix | nnz | nnx | velpn] ints
  size_t nd = pn * n + 4 * (size_t)n + 361 * (size_t)ncol + st.size() + n;
  size_t ni = pn * n + 5 * (size_t)n;
  double* dd = nullptr;
  int* di = nullptr;
  HIPCHK(dalloc(&dd, nd));
  if (hipMalloc((void**)&di, ni * 4) != hipSuccess) {
    dfree(dd);
    return fail(ctx, ALIFMM_E_HIP, "local_ops: out of memory");
  }
  double* p = dd;
  af::LocalOpsParams P;
  memset(&P, 0, sizeof P);
  P.op = op;
  P.n = n;
  P.pz = pz;
  P.px = px;
  hipError_t e = hipSuccess;
  auto putd = [&](const double* h, size_t cnt) {
    double* q = p;
    if (e == hipSuccess && cnt) e = hipMemcpy(q, h, cnt * 8, hipMemcpyHostToDevice);
    p += cnt;
    return (const double*)q;
  };
  P.ttn = putd(ttn, pn * n);
  P.cveln = putd(cell_veln, n);
  P.cvm = putd(cell_vm, n);
  P.dnx = putd(dnx, n);
  P.dnz = putd(dnz ? dnz : dnx, n);
  P.tab = putd(tab, 361 * (size_t)ncol);
  P.cstif = cell_stif ? putd(st.data(), st.size()) : nullptr;
  P.out = p;
  int* q = di;
  auto puti = [&](const int32_t* h, size_t cnt) {
    int* r = q;
    if (e == hipSuccess && cnt) e = hipMemcpy(r, h, cnt * 4, hipMemcpyHostToDevice);
    q += cnt;
    return (const int*)r;
  };
  P.nsts = puti(nsts, pn * n);
  P.iz = puti(iz, n);
  P.ix = puti(ix, n);
  P.nnz_arg = puti(nnz_arg, n);
  P.nnx_arg = puti(nnx_arg, n);
  P.cvelpn = puti(vp.data(), n);
  P.ncol = ncol;
  if (e == hipSuccess) e = af_launch_local_ops(&P, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, P.out, 8 * (size_t)n, hipMemcpyDeviceToHost);
  dfree(dd);
  dfree(di);
  if (e != hipSuccess) return fail(ctx, ALIFMM_E_HIP, "local_ops: %s", hipGetErrorString(e));
  return ALIFMM_OK;
}

int alifmm_fouds18_band(alifmm_ctx* ctx, int n, int pz, int px, const double* ttn, const int32_t* nsts,
                        const int32_t* iz, const int32_t* ix, const double* dnx, const double* dnz,
                        const int32_t* nnz_arg, const int32_t* nnx_arg, const int32_t* mz, const int32_t* mx, int quant,
                        double* out) {
  if (!ctx || !ctx->have_model || n < 0 || pz < 1 || px < 1 || (quant != 0 && quant != 1))
    return fail(ctx, ALIFMM_E_ARG, "fouds18_band: bad args or no model");
  if (!ctx->d_mid || !ctx->d_mslo)
    return fail(ctx, ALIFMM_E_ARG, "fouds18_band: the model has no per-material table (too many materials)");
  for (int k = 0; k < n; k++)
    if (mz[k] < 0 || mz[k] >= ctx->nz0 || mx[k] < 0 || mx[k] >= ctx->nx0)
      return fail(ctx, ALIFMM_E_ARG, "fouds18_band: model cell %d (%d, %d) outside the grid", k, mz[k], mx[k]);
  if (n == 0) return ALIFMM_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t pn = (size_t)pz * px;
  // [ttn | dnx | dnz | out] doubles, [nsts | iz | ix | nnz | nnx | mz | mx] ints
  double* dd = nullptr;
  int* di = nullptr;
  HIPCHK(dalloc(&dd, pn * n + 3 * (size_t)n));
  if (hipMalloc((void**)&di, (pn * n + 6 * (size_t)n) * 4) != hipSuccess) {
    dfree(dd);
    return fail(ctx, ALIFMM_E_HIP, "fouds18_band: out of memory");
  }
  af::LocalOpsParams P;
  memset(&P, 0, sizeof P);
  P.op = 2;
  P.n = n;
  P.pz = pz;
  P.px = px;
  P.RM = dev_model(ctx);
  P.quant = quant;
  hipError_t e = hipSuccess;
  double* p = dd;
  auto putd = [&](const double* h, size_t cnt) {
    double* q = p;
    if (e == hipSuccess && cnt) e = hipMemcpy(q, h, cnt * 8, hipMemcpyHostToDevice);
    p += cnt;
    return (const double*)q;
  };
  int* q = di;
  auto puti = [&](const int32_t* h, size_t cnt) {
    int* r = q;
    if (e == hipSuccess && cnt) e = hipMemcpy(r, h, cnt * 4, hipMemcpyHostToDevice);
    q += cnt;
    return (const int*)r;
  };
  P.ttn = putd(ttn, pn * n);
  P.dnx = putd(dnx, n);
  P.dnz = putd(dnz ? dnz : dnx, n);
  P.out = p;
  P.nsts = puti(nsts, pn * n);
  P.iz = puti(iz, n);
  P.ix = puti(ix, n);
  P.nnz_arg = puti(nnz_arg, n);
  P.nnx_arg = puti(nnx_arg, n);
  P.mz = puti(mz, n);
  P.mx = puti(mx, n);
  if (e == hipSuccess) e = af_launch_local_ops(&P, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, P.out, 8 * (size_t)n, hipMemcpyDeviceToHost);
  dfree(dd);
  dfree(di);
  if (e != hipSuccess) return fail(ctx, ALIFMM_E_HIP, "fouds18_band: %s", hipGetErrorString(e));
  return ALIFMM_OK;
}

}  // extern "C"
