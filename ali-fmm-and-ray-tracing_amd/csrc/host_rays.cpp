// host_rays.cpp — rays through resident fields: alifmm_find_rays / alifmm_take_rays and the points
// they keep, and the back-wall echo paths between element pairs (alifmm_skip_pick / _skip_rays).
#include <chrono>
#include <cstring>
#include <map>
#include <unordered_map>

#include "host_internal.h"

// plane-search candidates per ray the ray kernel holds (rays.hip kMaxCand)
static const int kMaxRayCand = 256;
// ray point buffers larger than this are freed at the end of each alifmm_find_rays call
static const size_t kRayBufKeepBytes = (size_t)1 << 30;
// points kept by alifmm_find_rays(..., ALIFMM_KEEP_RAYS) for alifmm_take_rays
void release_kept_rays(alifmm_ctx* c) {
  for (auto& k : c->kept_dev) dfree(k.d);
  c->kept_dev.clear();
  std::vector<std::vector<double>>().swap(c->kept_rays);
  c->kept_pts = 0;
}
// the ray tracer's work buffers hold `rays` rays of max_pts points (kept across calls, regrown for a larger launch)
static int ensure_ray_bufs(alifmm_ctx* ctx, int rays, int max_pts) {
  auto& rb = ctx->rb;
  if (rb.off.n >= (size_t)rays && rb.ry.n >= (size_t)rays * max_pts) return ALIFMM_OK;  // (the last grown of each)
  rb = {};
  HIPCHK(rb.rx.grow((size_t)rays * max_pts));
  HIPCHK(rb.ry.grow((size_t)rays * max_pts));
  HIPCHK(rb.t.grow(rays));
  HIPCHK(rb.len.grow(rays));
  HIPCHK(rb.flags.grow(rays));
  HIPCHK(rb.jobs.grow(rays));
  HIPCHK(rb.off.grow(rays));
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

extern "C" int alifmm_find_rays(alifmm_ctx* ctx, int npairs, const int32_t* field_slot, const double* src_xy,
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
  if (rb.rx.n * 2 * sizeof(double) > kRayBufKeepBytes) rb = {};
  return rc;
}

extern "C" int alifmm_take_rays(alifmm_ctx* ctx, double* ray_xy, int64_t ray_xy_cap, int64_t* n_points) {
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
  HIPCHK(B.tab.grow(nf));
  HIPCHK(B.wiz.grow((size_t)nw));
  HIPCHK(B.wix.grow((size_t)nw));
  HIPCHK(B.row.grow(2 * np));
  HIPCHK(B.hit.grow(np));
  HIPCHK(B.pick.grow(np));
  HIPCHK(B.W.grow(nf * (size_t)nw));
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

extern "C" int alifmm_skip_pick(alifmm_ctx* ctx, int npairs, const int32_t* slot_a, const int32_t* slot_b, int nw,
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

extern "C" int alifmm_skip_rays(alifmm_ctx* ctx, int npairs, const int32_t* slot_a, const int32_t* slot_b, const double* a_xy,
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
  if (rb.rx.n * 2 * sizeof(double) > kRayBufKeepBytes) rb = {};
  return rc;
}
