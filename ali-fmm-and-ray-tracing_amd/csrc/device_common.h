// device_common.h — shared gfx950 device code for the ALI-FMM travel-time-field solver.
//
// The local operators below are the reference's arithmetic (Anis_TTF_rays.py, cited per
// function) in double precision, operation order preserved and compiled with
// -ffp-contract=off, so that a cell evaluated on the same neighbourhood matches the CPU
// oracle to the last bit except where the trigonometric functions differ from glibc's.
// AF_CRMATH (default 1): atan / sin / cos / tan are cr_math.h's correctly rounded ones (glibc's
// results on all but ~0.1 % of arguments, where glibc itself is off by just over half an ulp);
// 0: ocml's (~1 % of results an ulp away).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef AF_CRMATH
#define AF_CRMATH 1
#endif
#include "cr_math.h"
#if AF_CRMATH
#define AF_ATAN crm::atan
#define AF_SIN crm::sin
#define AF_COS crm::cos
#define AF_TAN crm::tan
#define AF_SINCOS crm::sincos
#else
#define AF_ATAN atan
#define AF_SIN sin
#define AF_COS cos
#define AF_TAN tan
#define AF_SINCOS sincos
#endif

#define AF_DEV __device__ __forceinline__

// Python float '%' and round(), and time_between_points()'s walk (TbpWalk): plain arithmetic shared
// with host programs
#include "tbp_walk.h"

namespace af {

// Global-memory accesses through pointers the compiler cannot prove global (pointers stored in
// device-side structs, e.g. BandSrc) would otherwise compile to flat_* instructions, whose
// completion also counts on lgkmcnt and so serialises them against every LDS access.
#define AF_GLOBAL __attribute__((address_space(1)))
template <class T>
AF_DEV T gld(const T* p) {
  return *(const AF_GLOBAL T*)p;
}
template <class T>
AF_DEV void gst(T* p, T v) {
  *(AF_GLOBAL T*)p = v;
}
// the same pointer with its global address space made visible (an addrspace cast round trip):
// plain loads and stores through it compile to global_* instead of flat_*
template <class T>
AF_DEV T* gptr(T* p) {
  return (T*)(AF_GLOBAL T*)p;
}
AF_DEV int gatomic_max(int* p, int v) { return __atomic_fetch_max((AF_GLOBAL int*)p, v, __ATOMIC_RELAXED); }
// sc1 (L1-bypassing load, write-through store) accesses for data another CU writes or reads
// within the same launch (MI355X_MICROARCH.md "inter-workgroup visibility": sc1 stores, drained
// with vmcnt(0) before the signal, read back with sc1 loads after the signal)
template <class T>
AF_DEV T gld_sc1(const T* p) {
  return __hip_atomic_load((AF_GLOBAL T*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
AF_DEV void gst_sc1(T* p, T v) {
  __hip_atomic_store((AF_GLOBAL T*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Hand-shake words between two wavefront roles of one workgroup (the exact walks' heap role and
// relax role): release stores, acquire polls.  A waiting role backs off between polls (s_sleep) so
// that it takes no issue slots and LDS cycles from the working one, and gives up after 1 << 28
// polls: a broken protocol ends as an error, not as a hang.
AF_DEV void role_post(int* w, int v) { __hip_atomic_store(w, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
AF_DEV int role_load(int* w) { return __hip_atomic_load(w, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }
AF_DEV bool role_await_value(int* w, int v) {  // false: timeout (the other role is gone)
  for (long spins = 0; role_load(w) != v; spins++) {
    __builtin_amdgcn_s_sleep(1);
    if (spins > (1L << 28)) return false;
  }
  return true;
}
AF_DEV bool role_await_at_least(int* w, int v) {  // false: timeout
  for (long spins = 0; role_load(w) < v; spins++) {
    __builtin_amdgcn_s_sleep(1);
    if (spins > (1L << 28)) return false;
  }
  return true;
}
AF_DEV int role_await_change(int* w, int last) {  // the next value != last, or -2 on timeout
  for (long spins = 0;; spins++) {
    const int v = role_load(w);
    if (v != last) return v;
    __builtin_amdgcn_s_sleep(1);
    if (spins > (1L << 28)) return -2;
  }
}

// value of lane l (wave-uniform l) for every lane: v_readlane into a scalar register, no LDS round
// trip (a __shfl from one lane is a ds_bpermute: an LDS round trip in the wave's dependent chain)
AF_DEV int bcast(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
AF_DEV unsigned long long bcast64(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// ---------------------------------------------------------------------------------------------
// Distinct per-cell material (veln, vel_map, velpn, stiffness row): the band kernel stages the
// table in LDS and reads one 4-byte id per cell instead of four arrays.
struct MatRec {
  double veln, vm;
  int velpn, sidx;  // sidx -1: stif_den is None
};

// Model resident in HBM (uploaded once per set_model, shared by every source on the GPU).
struct DevModel {
  int nz0, nx0;          // coarse grid
  const double* veln;    // orientation [deg]
  const int* velpn;      // material column (0 = stiffness)
  const double* vm;      // velocity scale
  const int* sidx;       // stiffness row index per cell, or nullptr when stif_den is None
  const double* stab;    // unique stiffness rows [n][5] (exact int64 values as doubles)
  int nstab;             // number of unique stiffness rows
  const double* gtab;    // group velocity table (361, ncol)
  const double* ptab;    // phase velocity table (361, ncol)
  int ncol;
  const int* mid;        // material id per cell (into mtab), or nullptr when there are too many
  const unsigned char* mid8;  // the same ids as bytes when nmat <= 256, else nullptr
  const unsigned char* mid8b; // mid8 in 8 x 16 bricks (one 128-byte line each; pitch mid8b_pitch
  int mid8b_pitch;            // bricks per brick row), or nullptr: the band kernel's subgrid-1 view
  const MatRec* mtab;
  int nmat;
  const double* mslo;     // per material and MatView::quant: fouds18_A()'s 4 slownesses [nmat][2][4], or nullptr
};

// Logical grid -> coarse cell: f = lo1 + (a + side1)/s1 ; c = lo2 + (f + side2)/s2
// (finer_grid_n nearest-neighbour refinement, :26-56; windows :1516-1529, :2191-2204).
struct MatView {
  int s1z, side1z, lo1z, s1x, side1x, lo1x;
  int s2, side2, lo2z, lo2x;
  int quant;  // finer_grid_n quantisation: veln -> int32 (trunc), vel_map -> float32
};

AF_DEV long mv_cell(const DevModel& M, const MatView& v, int iz, int ix) {
  int fz = v.lo1z + (iz + v.side1z) / v.s1z;
  int fx = v.lo1x + (ix + v.side1x) / v.s1x;
  int cz = v.lo2z + (fz + v.side2) / v.s2;
  int cx = v.lo2x + (fx + v.side2) / v.s2;
  return (long)cz * M.nx0 + cx;
}

// fouds18_A()'s four slownesses of cell (iz, ix)'s material under view v (DevModel::mslo,
// precomputed per material on the device), or nullptr when the model has no material table
AF_DEV const double* mat_slo(const DevModel& M, const MatView& v, int iz, int ix) {
  if (!M.mid || !M.mslo) return nullptr;
  return M.mslo + 8 * (long)gld(M.mid + mv_cell(M, v, iz, ix)) + 4 * (v.quant ? 1 : 0);
}

struct CellMat {
  double veln, vm;
  int velpn;
  const double* stif;  // nullptr => None
};

AF_DEV CellMat cell_mat(const DevModel& M, const MatView& v, int iz, int ix) {
  long c = mv_cell(M, v, iz, ix);
  CellMat r;
  double a = gld(M.veln + c);
  double b = gld(M.vm + c);
  r.veln = v.quant ? (double)(int)a : a;
  r.vm = v.quant ? (double)(float)b : b;
  r.velpn = gld(M.velpn + c);
  r.stif = M.sidx ? M.stab + 5 * (long)gld(M.sidx + c) : nullptr;
  return r;
}

// Table lookup, linear in 1-degree bins (:288-291, :1372-1375, :2951-2954).
AF_DEV double table_vel(const double* tab, int ncol, double eff, int col, double vm) {
  long a1 = (long)floor(eff);
  long a2 = (a1 + 1) % 180;
  double rem = eff - (double)a1;
  return vm * ((1 - rem) * tab[a1 * ncol + col] + rem * tab[a2 * ncol + col]);
}

// Closed-form 2D orthotropic Christoffel GROUP velocity (:294-315, group_vel :3542-3558).
// s[] holds exact integers, so double arithmetic reproduces the reference's int64 sums/products.
AF_DEV double christoffel_group(const double* s, double eff, double vm) {
  double sigma = s[4];
  double e90 = pymod(eff, 90);
  if (e90 < 0.01 || e90 > 90 - 0.01) {
    double lam = (fabs(pymod(eff, 180) - 90) < 1) ? s[2] : s[0];
    return 1000 * vm * sqrt(lam / sigma);
  }
  double c22 = s[0], c23 = s[1], c33 = s[2], c44 = s[3];
  double tan_ang = AF_TAN(eff * kDeg2Rad);
  double A = c22 + c33 - 2 * c44;
  double B = (c23 + c44) * (tan_ang - 1 / tan_ang);
  double C = c22 - c33;
  double disc = B * B + A * A - C * C;
  double pa;
  if (eff < 90)
    pa = pymod(AF_ATAN((-B - sqrt(disc)) / (C - A)), M_PI);
  else
    pa = pymod(AF_ATAN((-B + sqrt(disc)) / (C - A)), M_PI);
  double s2, c2;  // sin and cos of 2 pa from one reduction
  AF_SINCOS(2 * pa, &s2, &c2);
  double lam = 0.5 * (c2 * (c22 - c44) + s2 * (c23 + c44) * tan_ang + c22 + c44);
  return 1000 * vm * sqrt(lam / sigma) / AF_COS(eff * kDeg2Rad - pa);
}

// Christoffel PHASE velocity (update() :1400-1406).
AF_DEV double christoffel_phase(const double* s, double eff, double vm) {
  double sa, ca;
  AF_SINCOS(eff * kDeg2Rad, &sa, &ca);
  double A = ca * ca * s[0] + sa * sa * s[3];
  double B = ca * sa * (s[1] + s[3]);
  double C = ca * ca * s[3] + sa * sa * s[2];
  return 1000 * vm * sqrt((A + C + sqrt((A - C) * (A - C) + 4 * (B * B))) / (2 * s[4]));
}

// group velocity with the selector 'velpn != 0 or stif_den == None' (:287, :2950); gtab: the
// group-velocity table (M.gtab or a copy in LDS)
AF_DEV double group_vel_cell(const DevModel& M, const CellMat& c, double eff, const double* gtab) {
  if (c.velpn != 0 || c.stif == nullptr) return table_vel(gtab, M.ncol, eff, c.velpn, c.vm);
  return christoffel_group(c.stif, eff, c.vm);
}
AF_DEV double group_vel_cell(const DevModel& M, const CellMat& c, double eff) {
  return group_vel_cell(M, c, eff, M.gtab);
}

// Material sources of time_between_points() on the coarse grid (identity view): the model
// arrays in HBM, or the material-id bytes plus the distinct records, stiffness rows and group
// table staged in LDS by the kernel (the same values: the records are the model's).
struct MatGlobal {
  const DevModel& M;
  AF_DEV int id(int z, int x) const { return M.mid ? gld(M.mid + (long)z * M.nx0 + x) : -1; }
  AF_DEV CellMat cm(int, int z, int x) const {
    const MatView ident{1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0};
    return cell_mat(M, ident, z, x);
  }
  AF_DEV const double* gtab() const { return M.gtab; }
};
struct MatLds {
  const DevModel& M;
  const MatRec* mat;
  const double* stab;
  const double* gt;
  AF_DEV int id(int z, int x) const {
    const long c = (long)z * M.nx0 + x;
    return M.mid8 ? (int)gld(M.mid8 + c) : gld(M.mid + c);
  }
  AF_DEV CellMat cm(int id, int, int) const {
    const MatRec m = mat[id];
    return CellMat{m.veln, m.vm, m.velpn, m.sidx >= 0 ? stab + 5 * m.sidx : nullptr};
  }
  AF_DEV const double* gtab() const { return gt; }
};

// wavefront_angle_dist :1413-1460
template <class I>
AF_DEV void wad(I ix, I iz, I x1, I x2, I x3, I z1, I z2, I z3, double y1, double y2, double y3, double& angle,
                double& dist) {
  double a;
  if (y3 != y1) {
    a = (y2 - y1) / (y3 - y1);
  } else {
    angle = 0.0;
    dist = -1.0;
    return;
  }
  double xpos = (1 - a) * (double)x1 + a * (double)x3;
  double zpos = (1 - a) * (double)z1 + a * (double)z3;
  double dx = (double)x2 - xpos;
  double dz = (double)z2 - zpos;
  if (dx == 0)
    angle = 0.0;
  else
    angle = pymod(AF_ATAN(dz / dx) * kRad2Deg + 90, 180);
  dist = fabs(dz * (double)(x2 - ix) - dx * (double)(z2 - iz)) / sqrt(dx * dx + dz * dz);
}

// slowness of material record cm along a segment at angle [deg]
template <class MS>
AF_DEV double tbp_slowness(const DevModel& M, const MS& ms, const CellMat& cm, double angle) {
  double eff = pymod(cm.veln - angle, 180);
  double velocity = group_vel_cell(M, cm, eff, ms.gtab());
  return 1.0 / velocity;
}

template <class MS>
AF_DEV double tbp(const DevModel& M, const MS& ms, double x1, double x2, double y1, double y2, double dnx, int sg) {
  double section_time = 0.0;
  TbpWalk w;
  double angle;
  w.setup(x1, x2, y1, y2, sg, angle);
  w.begin();
  int last_id = -1;
  double slown = 0.0;
  while (!w.done()) {
    double nxv, nyv;
    w.piece(nxv, nyv);
    int y_pos, x_pos;
    w.cell(M, nxv, nyv, y_pos, x_pos);
    // the slowness depends on the cell only through its material record (the angle is fixed for
    // the segment), so consecutive pieces in the same material reuse it: the same value, without
    // the group-velocity evaluation (the per-cell material id identifies the record exactly)
    const int id = ms.id(y_pos, x_pos);
    if (id < 0 || id != last_id) {
      slown = tbp_slowness(M, ms, ms.cm(id, y_pos, x_pos), angle);
      last_id = id;
    }
    section_time += w.piece_time(nxv, nyv, dnx, slown);
    w.prev_x = nxv;
    w.prev_y = nyv;
  }
  return section_time;
}
AF_DEV double tbp(const DevModel& M, double x1, double x2, double y1, double y2, double dnx, int sg) {
  return tbp(M, MatGlobal{M}, x1, x2, y1, y2, dnx, sg);
}

}  // namespace af
