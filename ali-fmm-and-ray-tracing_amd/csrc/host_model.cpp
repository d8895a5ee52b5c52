// host_model.cpp — the resident model: set_model's host passes (velocity maximum, unique stiffness
// rows and materials, interface density) and uploads, field_shape, and the DevModel the kernels get.
#include <array>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <thread>

#include "host_internal.h"

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

extern "C" int alifmm_set_model(alifmm_ctx* ctx, int nnz, int nnx, const double* veln, const int64_t* velpn,
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
  HIPCHK(ctx->dm.veln.grow(n));
  HIPCHK(ctx->dm.vm.grow(n));
  HIPCHK(ctx->dm.velpn.grow(n));
  HIPCHK(ctx->dm.gtab.grow((size_t)361 * ncol));
  HIPCHK(ctx->dm.ptab.grow((size_t)361 * ncol));
  HIPCHK(hipMemcpy(ctx->dm.veln, veln, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->dm.vm, vel_map, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->dm.velpn, vp.data(), n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->dm.gtab, group_tab, (size_t)361 * ncol * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->dm.ptab, phase_tab, (size_t)361 * ncol * 8, hipMemcpyHostToDevice));
  if (stif_den) {
    HIPCHK(ctx->dm.sidx.grow(n));
    HIPCHK(ctx->dm.stab.grow(stab.size()));
    HIPCHK(hipMemcpy(ctx->dm.sidx, sidx.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->dm.stab, stab.data(), stab.size() * 8, hipMemcpyHostToDevice));
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
      HIPCHK(ctx->dm.mid.grow(n));
      HIPCHK(ctx->dm.mtab.grow(recs.size()));
      HIPCHK(hipMemcpy(ctx->dm.mid, mid.data(), n * 4, hipMemcpyHostToDevice));
      if (recs.size() <= 256) {  // byte ids: 4x fewer lines per material gather in the band kernels
        std::vector<unsigned char> m8(n);
        for_chunks(n, nth, [&](int, size_t lo, size_t hi) {
          for (size_t i = lo; i < hi; i++) m8[i] = (unsigned char)mid[i];
        });
        HIPCHK(ctx->dm.mid8.grow(n));
        HIPCHK(hipMemcpy(ctx->dm.mid8, m8.data(), n, hipMemcpyHostToDevice));
        // the same ids in 8 x 16 bricks (one 128-byte line each) for the band kernel's subgrid-1 view
        const int bp = (nnx + 15) / 16, bz = (nnz + 7) / 8;
        std::vector<unsigned char> mb((size_t)128 * bp * bz, 0);
        for_chunks((size_t)bz, std::min(nth, bz), [&](int, size_t b0, size_t b1) {  // brick rows
          for (int z = (int)b0 * 8; z < std::min(nnz, (int)b1 * 8); z++)
            for (int x = 0; x < nnx; x++)
              mb[(((size_t)(z >> 3) * bp + (x >> 4)) << 7) | ((z & 7) << 4) | (x & 15)] = m8[(size_t)z * nnx + x];
        }, n < 65536 ? SIZE_MAX : 1);
        HIPCHK(ctx->dm.mid8b.grow(mb.size()));
        HIPCHK(hipMemcpy(ctx->dm.mid8b, mb.data(), mb.size(), hipMemcpyHostToDevice));
        ctx->mid8b_pitch = bp;
      }
      HIPCHK(hipMemcpy(ctx->dm.mtab, recs.data(), recs.size() * sizeof(af::MatRec), hipMemcpyHostToDevice));
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
    HIPCHK(ctx->dm.mslo.grow(8 * (size_t)ctx->nmat));
    const af::DevModel M = dev_model(ctx);
    HIPCHK(af_launch_mat_slowness(&M, ctx->dm.mslo, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  ctx->have_model = true;
  return ALIFMM_OK;
}

extern "C" int alifmm_field_shape(alifmm_ctx* ctx, int subgrid, int* fnz, int* fnx) {
  if (!ctx || !ctx->have_model || subgrid < 1 || subgrid % 2 == 0)
    return fail(ctx, ALIFMM_E_ARG, "field_shape: no model or even subgrid %d", subgrid);
  *fnz = subgrid * (ctx->nz0 - 1) + 1;
  *fnx = subgrid * (ctx->nx0 - 1) + 1;
  return ALIFMM_OK;
}

af::DevModel dev_model(const alifmm_ctx* c) {
  af::DevModel M;
  M.nz0 = c->nz0;
  M.nx0 = c->nx0;
  M.veln = c->dm.veln;
  M.velpn = c->dm.velpn;
  M.vm = c->dm.vm;
  M.sidx = c->dm.sidx;
  M.stab = c->dm.stab;
  M.nstab = c->nstab;
  M.mid = c->dm.mid;
  M.mid8 = c->dm.mid8;
  M.mid8b = c->dm.mid8b;
  M.mid8b_pitch = c->mid8b_pitch;
  M.mtab = c->dm.mtab;
  M.nmat = c->nmat;
  M.mslo = c->dm.mslo;
  M.gtab = c->dm.gtab;
  M.ptab = c->dm.ptab;
  M.ncol = c->ncol;
  return M;
}
