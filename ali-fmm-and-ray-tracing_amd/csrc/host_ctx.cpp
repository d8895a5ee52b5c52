// host_ctx.cpp — the context's life and settings: create and destroy, the options, release_fields,
// version, device count, last error.
#include <cstring>

#include "host_internal.h"

extern char** environ;

std::atomic<int> g_live_ctx{0};

extern "C" const char* alifmm_version(void) { return "alifmm-mi355x 0.1 (gfx950)"; }

extern "C" int alifmm_device_count(int* n) {
  int k = 0;
  hipError_t e = hipGetDeviceCount(&k);
  if (e != hipSuccess) k = 0;
  *n = k;
  return e == hipSuccess ? ALIFMM_OK : ALIFMM_E_HIP;
}

extern "C" int alifmm_ctx_create(int device, alifmm_ctx** out) {
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

void free_model(alifmm_ctx* c) {
  c->op = {};  // the resident sensitivity operator belongs to the model it was built on
  c->dm = {};
  c->nmat = 0;
  c->have_model = false;
}

extern "C" int alifmm_release_fields(alifmm_ctx* ctx) {
  if (!ctx) return ALIFMM_E_ARG;
  (void)hipSetDevice(ctx->device);
  ctx->fields.clear();
  ctx->rb = {};  // the ray tracer's point buffers (chunk x max_pts per coordinate) go with the fields
  release_kept_rays(ctx);
  free_stream_bufs(ctx);  // the pinned staging of streamed fields too
  return ALIFMM_OK;
}

extern "C" int alifmm_ctx_destroy(alifmm_ctx* ctx) {
  if (!ctx) return ALIFMM_OK;
  g_live_ctx--;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  destroy_team(ctx);
  alifmm_release_fields(ctx);
  ctx->arena = {};
  ctx->all = {};
  ctx->ho_last = nullptr;
  ctx->seed = {};
  ctx->tfm = {};
  ctx->tfm_lsq = {};
  ctx->tfm_sparse = {};
  ctx->fir = {};
  ctx->fft = {};
  ctx->pick = {};
  ctx->tfm_model = {};
  ctx->skip = {};
  ctx->sens = {};
  ctx->solve = {};
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

extern "C" const char* alifmm_last_error(alifmm_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }

extern "C" int alifmm_set_option(alifmm_ctx* ctx, const char* name, double value) {
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

extern "C" int alifmm_get_option(alifmm_ctx* ctx, const char* name, double* value) {
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
  // last alifmm_tfm_sparse call: the same, the doublings of L, and the L its first iteration began with
  else if (!strcmp(name, "tfm_sparse_upload_ms")) *value = ctx->t_tfm_sparse_upload;
  else if (!strcmp(name, "tfm_sparse_kernel_ms")) *value = ctx->t_tfm_sparse_kernel;
  else if (!strcmp(name, "tfm_sparse_iters")) *value = ctx->tfm_sparse_iters;
  else if (!strcmp(name, "tfm_sparse_backtracks")) *value = ctx->tfm_sparse_backtracks;
  else if (!strcmp(name, "tfm_sparse_l0")) *value = ctx->tfm_sparse_l0;
  // last alifmm_trace_fir call (ms): host -> device copies (host clock), the kernel (HIP events); the
  // outputs per workgroup of the kernel (a constant of the build)
  else if (!strcmp(name, "trace_fir_upload_ms")) *value = ctx->t_fir_upload;
  else if (!strcmp(name, "trace_fir_kernel_ms")) *value = ctx->t_fir_kernel;
  else if (!strcmp(name, "trace_fir_tile")) *value = af_trace_fir_tile();
  // last alifmm_trace_spectral call (ms): host -> device copies (host clock), the kernel (HIP events),
  // the device -> host copy (host clock); the most workgroups a launch starts (a constant of the build)
  else if (!strcmp(name, "trace_fft_upload_ms")) *value = ctx->t_fft_upload;
  else if (!strcmp(name, "trace_fft_kernel_ms")) *value = ctx->t_fft_kernel;
  else if (!strcmp(name, "trace_fft_download_ms")) *value = ctx->t_fft_download;
  else if (!strcmp(name, "trace_fft_grid")) *value = af_trace_fft_grid();
  else if (!strcmp(name, "trace_pick_upload_ms")) *value = ctx->t_pick_upload;
  else if (!strcmp(name, "trace_pick_filter_ms")) *value = ctx->t_pick_filter;
  else if (!strcmp(name, "trace_pick_kernel_ms")) *value = ctx->t_pick_kernel;
  else if (!strcmp(name, "trace_pick_download_ms")) *value = ctx->t_pick_download;
  else if (!strcmp(name, "trace_pick_grid")) *value = af_trace_pick_grid();
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
