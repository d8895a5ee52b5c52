// host_fields.cpp — resident fields to and from the host: get_field / put_field, the copy team and
// the pinned staging ring (copy_fields, d2h_pageable), the host side of fields streamed out of the
// band kernel, and the per-field statistics and profiles.
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>

#include "host_internal.h"

// host copies up to this size go straight to pageable memory while the pinned ring is unallocated
static const size_t kSmallD2H = (size_t)64 << 20;
extern "C" int alifmm_get_field(alifmm_ctx* ctx, int slot, double* out) {
  if (!ctx || slot < 0 || slot >= (int)ctx->fields.size() || !ctx->fields[slot].d || !out)
    return fail(ctx, ALIFMM_E_ARG, "get_field: no field in slot %d", slot);
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(out, ctx->fields[slot].d, ctx->fields[slot].bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ALIFMM_OK;
}

extern "C" int alifmm_put_field(alifmm_ctx* ctx, int slot, int subgrid, const double* data) {
  if (!ctx || !ctx->have_model || slot < 0 || !data) return fail(ctx, ALIFMM_E_ARG, "put_field: bad args");
  int fz, fx;
  int rc = alifmm_field_shape(ctx, subgrid, &fz, &fx);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  if ((rc = af_ensure_field(ctx, slot, subgrid, fz, fx))) return rc;
  HIPCHK(hipMemcpy(ctx->fields[slot].d, data, (size_t)fz * fx * 8, hipMemcpyHostToDevice));
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
void destroy_team(alifmm_ctx* ctx) {
  delete static_cast<CopyTeam*>(ctx->team);
  ctx->team = nullptr;
}

void free_stream_bufs(alifmm_ctx* ctx) {
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
int stream_setup(alifmm_ctx* ctx, StreamOut* so, int n, int K, int wlog, int fz, int fx) {
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

void stream_start(alifmm_ctx* ctx, StreamOut* so) {
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
void stream_finish(alifmm_ctx* ctx, StreamOut* so) {
  const auto t0 = std::chrono::steady_clock::now();
  so->kernel_done.store(1, std::memory_order_release);
  copy_team(ctx).wait();
  ctx->t_stream_tail += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Device -> pageable host copy of a list of segments: pieces of kPinBytes through kPinBufs pinned
// buffers; the DMA of the next pieces runs while a thread team copies the current one out of its
// buffer (alifmm_copy_fields, alifmm_take_rays)
int d2h_pageable(alifmm_ctx* ctx, const std::vector<D2HSeg>& segs) {
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

extern "C" int alifmm_copy_fields(alifmm_ctx* ctx, int first_slot, int n, double* dst, int dst_kind, double* gbps) {
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
    for (int i = 0; i < n; i++) segs[i] = {(const char*)ctx->fields[first_slot + i].d.p, out + (size_t)i * fb, fb};
    const int rc = d2h_pageable(ctx, segs);
    if (rc) return rc;
  }
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (gbps) *gbps = dt > 0 ? (double)fb * n / dt / 1e9 : 0.0;
  return ALIFMM_OK;
}

extern "C" int alifmm_source_stats(alifmm_ctx* ctx, int slot, int64_t* steps4, int64_t* cell_sweeps) {
  if (!ctx || slot < 0 || slot >= (int)ctx->fields.size()) return fail(ctx, ALIFMM_E_ARG, "stats: bad slot");
  if (steps4)
    for (int k = 0; k < 4; k++) steps4[k] = ctx->fields[slot].steps[k];
  if (cell_sweeps) *cell_sweeps = ctx->fields[slot].sweeps;
  return ALIFMM_OK;
}

extern "C" int alifmm_band_profile(alifmm_ctx* ctx, int slot, int64_t* out14) {
  if (!ctx || slot < 0 || slot >= (int)ctx->fields.size() || !out14) return fail(ctx, ALIFMM_E_ARG, "band_profile: bad slot");
  for (int k = 0; k < 14; k++) out14[k] = ctx->fields[slot].prof[k];
  return ALIFMM_OK;
}

extern "C" int alifmm_band_span(alifmm_ctx* ctx, int slot, int64_t* out2) {
  if (!ctx || slot < 0 || slot >= (int)ctx->fields.size() || !out2) return fail(ctx, ALIFMM_E_ARG, "band_span: bad slot");
  out2[0] = ctx->fields[slot].span[0];
  out2[1] = ctx->fields[slot].span[1];
  return ALIFMM_OK;
}

extern "C" int alifmm_init_profile(alifmm_ctx* ctx, int i, int64_t* out16) {
  if (!ctx || !out16 || i < 0 || i >= ctx->n_ho_last || !ctx->ho_last)
    return fail(ctx, ALIFMM_E_ARG, "init_profile: bad index");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpy(out16, &ctx->ho_last[i].prof[0], 16 * sizeof(long long), hipMemcpyDeviceToHost));
  return ALIFMM_OK;
}

extern "C" int alifmm_last_timing(alifmm_ctx* ctx, double* init_ms, double* band_ms, double* total_ms) {
  if (!ctx) return ALIFMM_E_ARG;
  if (init_ms) *init_ms = ctx->t_init;
  if (band_ms) *band_ms = ctx->t_band;
  if (total_ms) *total_ms = ctx->t_total;
  return ALIFMM_OK;
}
