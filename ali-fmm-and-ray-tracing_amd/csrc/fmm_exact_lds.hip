// fmm_exact_lds.hip — travel_finer_grid()'s exact heap walk (the x9 / x3 stage grids
// Anis_TTF_rays.py:2187-2504 and the fine-grid main loop's prefix :2775-2817) with the walk's
// state in LDS, on gfx950.
//
// fmm_exact.hip keeps the walk's statuses (nsts) in HBM next to the grids, so every pop pays
// memory round trips on its serial path: the neighbours' statuses, the heap index of an updated
// node, the 12-point stencil of a relaxation whose speculative entry went stale, and a store
// drain per relaxation (≈7.7 µs per pop on the weld example, 50 % of the wave's cycles waiting,
// profiles/r4exact_*).  Here only the travel times stay in HBM; everything the walk decides on
// is in LDS:
//   * statuses as 2-bit codes (far / close / known) of every node of the current grid (stage
//     grids whole, up to 163 840 nodes = subgrid 9; the fine main grid as a window around the
//     source that covers the prefix);
//   * the heap (keys = copies of ttn, as in fmm_exact.hip) with, per entry, the node and the slot
//     of the node's heap index in an LDS hash (node -> the reference's nsts > 0), so sifts write
//     heap indices without a lookup;
//   * per lane, a speculative relaxation (node, value, update()'s stencil stage, material) whose
//     12-point stencil is kept current in LDS: every committed relaxation patches the stencils
//     that contain its node, so a stale entry is re-checked (stencil stage re-run, finish only if
//     it changed) without any memory access.  Only relaxations with no entry cost a memory round
//     trip: one evaluation pass in which lane 0 evaluates the job and the other lanes guesses (the
//     neighbours of the heap's first 16 entries), as in fmm_exact.hip.
// The walk, its heap (walk_heap.h, shared), duplicate entries (the stage-1 window corners,
// :2277-2288) and the hand-over order are fmm_exact.hip's, which reproduces the reference's;
// results are bit-identical to it (tests/test_gpu_parity.py weld sg 3 / 9 fields,
// tools/weld_split.py --dump).  Larger grids (subgrid > 9) and heap overflows use fmm_exact.hip.
#define CR_LDS_TABLES  // cr_math.h tables in LDS (crm::lds_init at kernel start)
#include "kernels.h"
#include "local_ops.h"
#include "fields.h"
#include "walk_heap.h"
#include "walk_rules.h"

namespace af {
namespace xl {

constexpr int kThreads = 256;  // 4 waves clear and hand over; wave 0 walks
#ifndef AF_XL_DIAG
#define AF_XL_DIAG 0  // diagnostic build: cycle counters of the two roles (BandSrc::ph)
#endif
constexpr int kCap = 163840;   // status nodes (2 bits each): stage grids up to 404 x 404
constexpr int kHeap = 4096;    // heap slots (1-based)
constexpr int kHTLog = 13;
constexpr int kHT = 1 << kHTLog;  // hash slots (node -> heap index)
constexpr int kDec = 18432;       // decimated nodes of a stage grid (hand-over classes)
constexpr int kDup = 8;           // nodes with two heap entries

constexpr unsigned kSFar = kWalkFar, kSClose = kWalkClose, kSKnown = kWalkKnown;  // 2-bit status codes

struct Lds {
  unsigned st[kCap / 16];
  double key[kHeap];
  unsigned ent[kHeap];
  unsigned ht[kHT];
  double stn[12][64];  // per-lane speculative stencils, [stencil slot][lane]
  signed char dec[kDec];
  int dup[kDup];
  int nused;  // hash slots that are live or tombstones
  // two-role walk (heap wavefront -> relax wavefront): command sequence number (-1 stop), the
  // pop's relaxation jobs (node | fresh << 31), relaxations done / applied to the heap (running
  // counts), their values, the heap size (for the relax role's guesses), serial (see heap_role)
  int cmd, done, applied, njob, serial, ntr_hint;
  int job[4];
  double jval[4];
};
static_assert(sizeof(Lds) == 147568, "the LDS layout is fixed: the walk has no room to spare");

AF_DEV unsigned sget(const Lds* L, int c) { return (L->st[c >> 4] >> ((c & 15) * 2)) & 3u; }
AF_DEV void sset(Lds* L, int c, unsigned v) {  // any previous state (LDS atomics: lanes share words)
  const unsigned sh = (c & 15) * 2;
  atomicAnd(&L->st[c >> 4], ~(3u << sh));
  if (v) atomicOr(&L->st[c >> 4], v << sh);
}

// the grid of a walk: T in HBM (row-major nz x nx, far = NaN), statuses of the window rows
// [wz0, wz0 + wh), columns [wx0, wx0 + ww) in LDS (stage grids: the whole grid)
struct XG {
  double* T;
  int nz, nx;
  int wz0, wx0, wh, ww;
  MatView mv;
  double dnx, dnz;
  AF_DEV bool inw(int z, int x) const { return z >= wz0 && z < wz0 + wh && x >= wx0 && x < wx0 + ww; }
  AF_DEV int loc(int z, int x) const { return (z - wz0) * ww + (x - wx0); }
  AF_DEV int gz(int c) const { return wz0 + c / ww; }
  AF_DEV int gx(int c) const { return wx0 + c % ww; }
};

// status accessor for fouds18_A() (known = 0, close = 1, far = -1) with T from HBM (far -> 0)
struct XField {
  const Lds* L;
  const XG* g;
  AF_DEV int st(long z, long x) const {
    if (z >= g->nz || !g->inw((int)z, (int)x)) return -1;
    const unsigned s = sget(L, g->loc((int)z, (int)x));
    return s == kSKnown ? 0 : s == kSClose ? 1 : -1;
  }
  AF_DEV double tt(long z, long x) const {
    if (z >= g->nz || z < 0 || x < 0 || x >= g->nx) return 0.0;
    return far0(gld(g->T + z * g->nx + x));
  }
};

// The heap (walk_heap.h) with its heap indices (nsts > 0) in the LDS hash (WalkHashStore).  Lane 0
// only.  The store's device side: the status codes' accesses, and both reads of a heap slot kept
// in one LDS round trip (not the entry after the key's compare).
struct HeapDev {
  Lds* L;
  AF_DEV unsigned get(int c) const { return sget(L, c); }
  AF_DEV void set(int c, unsigned v) const { sset(L, c, v); }
  AF_DEV void pin(unsigned& e) const { asm volatile("" : "+v"(e)); }
  AF_DEV void pin(unsigned& e1, unsigned& e2) const { asm volatile("" : "+v"(e1), "+v"(e2)); }
};
using HeapStore = WalkHashStore<Lds, HeapDev, kHTLog>;
// the store's words, which rehash() and the kernel's outputs read: hash words live | pos << 18 |
// node, heap entries node | hash slot << 18 | kDupF
constexpr unsigned kLive = HeapStore::kLive, kTomb = HeapStore::kTomb, kNodeM = HeapStore::kNodeM,
                   kDupF = HeapStore::kDupF;
static_assert(kHeap <= 1 << 12 && kCap <= 1 << 18 && kHTLog <= 13, "the words' fields hold them");
struct Heap : WalkHeap<HeapStore, kHeap, kDup, 9> {
  AF_DEV explicit Heap(Lds* L) {
    s.m = L;
    s.dev.L = L;
  }
  using WalkHeap::upd;
  AF_DEV void upd(int c, double key) {
    const int tpc = s.pos_of(c);
    upd(tpc, s.m->ent[tpc], key);
  }
  // pop the root in two parts: its status -> known; then its heap-index slot freed (unless the
  // node has another entry) and downtree
  AF_DEV void pop_known() { sset(s.m, (int)(s.m->ent[1] & kNodeM), kSKnown); }
  AF_DEV void pop_rest() {
    s.leave(s.m->ent[1]);
    pop_down();
  }
};

// Rebuild the hash without its tombstones (wave 0, every lane): each heap entry's node is
// re-inserted with the heap index of that entry (nodes with two entries: the index the old slot
// held) and the entry takes the new slot.
AF_DEV void rehash(Lds* L, Heap& h, int lane) {
  int ntr = __shfl(h.ntr, 0), nd = __shfl(h.ndup, 0);
  // the heap indices of the nodes with two entries, before the table is cleared
  int dpos = -1, dnode = -1;
  if (lane < nd) {
    dnode = L->dup[lane];
    unsigned s = HeapStore::hslot(dnode);
    for (int p = 0; p < kHT; p++) {
      const unsigned w = L->ht[s];
      if (w == 0u) break;
      if ((w >> 30) == 1u && (int)(w & kNodeM) == dnode) {
        dpos = (int)((w >> 18) & 0xfffu);
        break;
      }
      s = (s + 1) & (kHT - 1);
    }
  }
  for (int k = lane; k < kHT; k += 64) L->ht[k] = 0u;
  for (int k = 1 + lane; k <= ntr; k += 64) {
    const unsigned e = L->ent[k];
    const int c = (int)(e & kNodeM);
    unsigned s = HeapStore::hslot(c);
    while (true) {
      const unsigned prev = atomicCAS(&L->ht[s], 0u, kLive | ((unsigned)k << 18) | (unsigned)c);
      if (prev == 0u || (int)(prev & kNodeM) == c) break;
      s = (s + 1) & (kHT - 1);
    }
    L->ent[k] = (e & ~(((unsigned)(kHT - 1)) << 18)) | (s << 18);
  }
  // popped nodes with two entries keep a slot even with no entry left
  if (lane < nd && dpos >= 0) {
    unsigned s = HeapStore::hslot(dnode);
    while (true) {
      const unsigned prev = atomicCAS(&L->ht[s], 0u, kLive | ((unsigned)dpos << 18) | (unsigned)dnode);
      if (prev == 0u) break;
      if ((int)(prev & kNodeM) == dnode) {
        L->ht[s] = kLive | ((unsigned)dpos << 18) | (unsigned)dnode;
        break;
      }
      s = (s + 1) & (kHT - 1);
    }
  }
  int used = 0;
  for (int k = lane; k < kHT; k += 64) used += L->ht[k] != 0u;
  for (int o = 32; o > 0; o >>= 1) used += __shfl_xor(used, o);
  if (lane == 0) L->nused = used;
}

// One lane's speculative relaxation: node (window-local, -1: none), grid coordinates, value,
// update()'s stencil stage and the node's material; its stencil values live in Lds::stn.
struct Spec {
  int c, z, x;
  unsigned vm;
  bool dirty;
  double v;
  UpdSel sel;
  CellMat cm;
};

// every lane: committed relaxation (rz, rx) = v -> the stencils that contain it
AF_DEV void patch(Lds* L, Spec& sp, int rz, int rx, double v, int lane) {
  if (sp.c < 0) return;
  const int dz = rz - sp.z, dx = rx - sp.x;
  if (!stencil_holds(dz, dx)) return;
  const int k = NbField::slot(dz, dx);
  L->stn[k][lane] = v;
  sp.vm |= 1u << k;
  sp.dirty = true;
}

AF_DEV void stencil_from_lds(const Lds* L, const Spec& sp, NbFieldT& nb, int lane) {
  nb.iz = sp.z;
  nb.ix = sp.x;
  nb.vm = sp.vm;
  nb.t0 = L->stn[0][lane]; nb.t1 = L->stn[1][lane]; nb.t2 = L->stn[2][lane]; nb.t3 = L->stn[3][lane];
  nb.t4 = L->stn[4][lane]; nb.t5 = L->stn[5][lane]; nb.t6 = L->stn[6][lane]; nb.t7 = L->stn[7][lane];
  nb.t8 = L->stn[8][lane]; nb.t9 = L->stn[9][lane]; nb.t10 = L->stn[10][lane]; nb.t11 = L->stn[11][lane];
}

// update() of the job (rz, rx) on the current state (wave 0, every lane; wave-uniform result).
// An entry for the node: its stencil is current (patched), so its value stands if the stencil
// stage is unchanged, else the finish runs on the entry's lane.  No entry: one evaluation pass —
// the job on lane 0, and on every other lane a guess (a neighbour of one of the heap's first 16
// entries that is not known), each loading its stencil and material from memory.
AF_DEV double relax_value(Lds* L, const DevModel& M, const XG& g, Spec& sp, int r, int rz, int rx, int ntr,
                          int lane, long long& npass) {
  const unsigned long long hm = __ballot(sp.c == r);
  if (hm) {
    const int e = __ffsll((long long)hm) - 1;
    if (__builtin_amdgcn_readlane((int)sp.dirty, e)) {
      // the patched stencil's stage again, spread over the wavefront (lane k < 12: slot k of the
      // entry's stencil; lanes 0..7 a square stencil each), on the entry's lane where update()
      // runs its triangular stage
      const unsigned vm_e = (unsigned)__builtin_amdgcn_readlane((int)sp.vm, e);
      const int z_e = __builtin_amdgcn_readlane(sp.z, e), x_e = __builtin_amdgcn_readlane(sp.x, e);
      const double tk = lane < 12 ? L->stn[lane][e] : 0.0;
      const bool vk = lane < 12 && ((vm_e >> lane) & 1u);
      UpdSel s2;
      const bool par = update_select_lanes(tk, vk, z_e, x_e, g.nz, g.nx, lane, s2);
      if (lane == e) {
        if (!par) {
          NbFieldT nb;
          stencil_from_lds(L, sp, nb, lane);
          s2 = update_nb_select(nb, sp.z, sp.x, g.nz, g.nx);
        }
        if (!s2.same(sp.sel)) {
          sp.v = update_nb_finish_ool(M, sp.cm, sp.z, sp.x, g.dnx, s2);
          sp.sel = s2;
        }
        sp.dirty = false;
      }
    }
    return lane_d(sp.v, e);
  }
  npass++;
  int cz = rz, cx = rx;
  bool cand = true;
  if (lane > 0) {
    const WalkGuess gs = walk_guess(lane);
    const int hc = (int)(L->ent[gs.entry] & kNodeM);
    const WalkNode q = walk_nbr(gs.dir, g.gz(hc), g.gx(hc));
    cz = q.z;
    cx = q.x;
    cand = gs.entry <= ntr && cz >= 0 && cz < g.nz && cx >= 0 && cx < g.nx && g.inw(cz, cx) &&
           sget(L, g.loc(cz, cx)) != kSKnown;
  }
  if (cand) {
    sp.cm = cell_mat(M, g.mv, cz, cx);
    NbFieldT nb;
    nb.load(g.T, g.nz, g.nx, cz, cx);
    L->stn[0][lane] = nb.t0; L->stn[1][lane] = nb.t1; L->stn[2][lane] = nb.t2; L->stn[3][lane] = nb.t3;
    L->stn[4][lane] = nb.t4; L->stn[5][lane] = nb.t5; L->stn[6][lane] = nb.t6; L->stn[7][lane] = nb.t7;
    L->stn[8][lane] = nb.t8; L->stn[9][lane] = nb.t9; L->stn[10][lane] = nb.t10; L->stn[11][lane] = nb.t11;
    sp.vm = nb.vm;
    sp.sel = update_nb_select(nb, cz, cx, g.nz, g.nx);
    sp.v = update_nb_finish_ool(M, sp.cm, cz, cx, g.dnx, sp.sel);
    sp.c = g.loc(cz, cx);
    sp.z = cz;
    sp.x = cx;
    sp.dirty = false;
  } else {
    sp.c = -1;
  }
  return lane_d(sp.v, 0);
}

// ---- the heap walk (:2292-2346, :2460-2504, :2775-2817) over two wavefronts ----
// stage: stop when a popped node's neighbour falls off the stage grid at max_dist + 1 from the
// source; main grid: stop when the root reaches tstop or comes within 3 nodes of a window edge
// that is not a grid edge.
// The heap wavefront pops, classifies the popped node's neighbours (far -> addtree, close ->
// updtree, statuses read before downtree as in fmm_exact.hip), makes the node known and hands the
// relaxation jobs to the relax wavefront, then runs downtree while the relaxations are evaluated,
// and each job's addtree / updtree as soon as its value is posted.  The relax wavefront evaluates
// the jobs in order (speculative entries / evaluation passes / fouds18_A(), relax_value) and
// stores T.  update() reads T and validity only, which neither downtree nor addtree / updtree
// change, so the values are those of a walk on one wavefront.  fouds18_A() reads known-ness, which
// the heap side changes only through a node with two heap entries (setpos makes it close again):
// while such entries are in the heap (Heap::livedup) the heap runs downtree before posting the
// jobs and the relax side waits for the earlier jobs' addtree / updtree before a fouds18_A() —
// the sequential order.

// heap wavefront (every lane; lane 0 holds the heap).  Returns the pops.
AF_DEV long long heap_role(Lds* L, Heap& h, const XG& g, bool stage, int isx_s, int isz_s, int max_dist,
                           double tstop, int lane, long long* dgo) {
  long long pops = 0;
  long long dg[4] = {0, 0, 0, 0};  // AF_XL_DIAG: waits for relaxations, downtree, addtree / updtree, the rest
  long long tl = AF_XL_DIAG ? clock64() : 0;
  bool finished = false;
  int seq = 0, jobs = 0;
  while (true) {
    int go = 0, c = 0;
    if (lane == 0) {
      if (L->nused > (kHT * 3) / 4) go = -1;  // rehash first
      else go = h.ntr > 0 && !finished && !h.err && !(tstop > 0 && L->key[1] >= tstop);
      c = (int)(L->ent[1] & kNodeM);
    }
    go = __shfl(go, 0);
    if (go < 0) {
      rehash(L, h, lane);
      continue;
    }
    if (!go) break;
    c = __shfl(c, 0);
    const int iz = g.gz(c), ix = g.gx(c);
    if (!stage && ((g.wz0 > 0 && iz - g.wz0 < 3) || (g.wz0 + g.wh < g.nz && g.wz0 + g.wh - 1 - iz < 3) ||
                   (g.wx0 > 0 && ix - g.wx0 < 3) || (g.wx0 + g.ww < g.nx && g.wx0 + g.ww - 1 - ix < 3))) {
      // the window edge before tstop (the root key is still below it): the HBM walk redoes the
      // source (error 9), so the hand-over is the reference's prefix to tstop
      if (lane == 0) h.err = 9;
      break;
    }
    const WalkNode nb4 = walk_nbr(lane & 3, iz, ix);
    const bool inb = lane < 4 && walk_in_grid(lane & 3, nb4, g.nz, g.nx);
    const unsigned st = inb ? sget(L, g.loc(nb4.z, nb4.x)) : kSKnown;
    const bool edge = lane < 4 && !inb && stage && walk_stage_stop(lane & 3, nb4, isz_s, isx_s, max_dist);
    const unsigned long long jm = __ballot(inb && st != kSKnown);
    if (__ballot(edge) != 0ull) finished = true;
    const unsigned long long fm = __ballot(inb && st == kSFar);
    const int n = __popcll(jm);
    pops++;
    if (lane == 0) {
      h.pop_known();  // the popped node is known before any relaxation of this pop (fouds18_A)
      const bool serial = h.s.livedup > 0;
      if (serial || n == 0) h.pop_rest();
      if (n > 0) {
        int q = 0;
        for (int k = 0; k < 4; k++) {
          if (!((jm >> k) & 1ull)) continue;
          const WalkNode rn = walk_nbr(k, iz, ix);
          L->job[q++] = g.loc(rn.z, rn.x) | (((fm >> k) & 1ull) ? (int)0x80000000 : 0);
        }
        L->njob = n;
        L->serial = serial ? 1 : 0;
        L->ntr_hint = h.ntr;
        role_post(&L->cmd, ++seq);
        long long t1 = AF_XL_DIAG ? clock64() : 0;
        if (AF_XL_DIAG) dg[3] += t1 - tl;
        if (!serial) h.pop_rest();  // downtree beside the relaxations
        if (AF_XL_DIAG) {
          const long long t2 = clock64();
          dg[1] += t2 - t1;
          t1 = t2;
        }
        for (int q2 = 0; q2 < n; q2++) {
          if (!role_await_at_least(&L->done, jobs + q2 + 1)) {
            h.err = 10;
            break;
          }
          long long t3 = AF_XL_DIAG ? clock64() : 0;
          if (AF_XL_DIAG) dg[0] += t3 - t1;
          const int jw = L->job[q2];
          const int r = jw & 0x7fffffff;
          const double v = L->jval[q2];
          if (jw < 0) h.add(r, v, true);
          else h.upd(r, v);
          role_post(&L->applied, jobs + q2 + 1);
          if (AF_XL_DIAG) {
            t1 = clock64();
            dg[2] += t1 - t3;
          }
        }
        if (AF_XL_DIAG) tl = t1;
        jobs += n;
      }
    }
  }
  if (lane == 0) role_post(&L->cmd, -1);
  if (AF_XL_DIAG && lane == 0)
    for (int k = 0; k < 4; k++) dgo[k] += dg[k];
  return pops;
}

// relax wavefront (every lane)
AF_DEV void relax_role(Lds* L, const DevModel& M, const XG& g, Spec& sp, int lane, long long* prof,
                       long long* dgo) {
  long long nrel = 0, npass = 0;
  long long dg[2] = {0, 0};  // AF_XL_DIAG: waits for a command, the rest
  int last = 0, jobs = 0;
  sp.c = -1;
  while (true) {
    int cmd = 0;
    const long long tw = AF_XL_DIAG ? clock64() : 0;
    if (lane == 0) cmd = role_await_change(&L->cmd, last);
    cmd = __shfl(cmd, 0);
    const long long tw2 = AF_XL_DIAG ? clock64() : 0;
    if (AF_XL_DIAG) dg[0] += tw2 - tw;
    if (cmd < 0) break;  // stop (or timeout: the heap wavefront is gone)
    last = cmd;
    const int n = L->njob, serial = L->serial, ntr = L->ntr_hint;
    const int4 jv = *reinterpret_cast<const int4*>(L->job);
    for (int q = 0; q < n; q++) {
      const int jw = q == 0 ? jv.x : q == 1 ? jv.y : q == 2 ? jv.z : jv.w;
      const int r = jw & 0x7fffffff;
      const int rz = g.gz(r), rx = g.gx(r);
      double v = relax_value(L, M, g, sp, r, rz, rx, ntr, lane, npass);
      nrel++;
      if (lane == 0) {
        if (v == -1.0) {
          if (serial) role_await_at_least(&L->applied, jobs + q);  // the earlier jobs' heap updates first
          const XField F{L, &g};
          v = fouds18(F, M, cell_mat(M, g.mv, rz, rx), rz, rx, g.dnx, g.dnz, g.nx, g.nz, mat_slo(M, g.mv, rz, rx));
        }
        gst(g.T + (long)rz * g.nx + rx, v);
        L->jval[q] = v;
        role_post(&L->done, jobs + q + 1);
      }
      v = lane_d(v, 0);
      patch(L, sp, rz, rx, v, lane);
    }
    jobs += n;
    if (AF_XL_DIAG) dg[1] += clock64() - tw2;
  }
  if (prof && lane == 0) {
    prof[0] += nrel;
    prof[1] += npass;
  }
  if (AF_XL_DIAG && lane == 0) {
    dgo[4] += dg[0];
    dgo[5] += dg[1];
  }
}

// all threads: the hand-over class of every 3rd node of the grid just walked (:2391-2425,
// :2725-2759): 0 far, 1 known, 2 known with a far (or missing) node 3 away = "outer", 3 close
AF_DEV void classify(Lds* L, int nz, int nx, int tid) {
  const int dz = (nz - 1) / 3 + 1, dx = (nx - 1) / 3 + 1;
  for (int k = tid; k < dz * dx; k += kThreads) {
    const int i = 3 * (k / dx), j = 3 * (k % dx);
    // the 2-bit codes as the reference's statuses: far -1, known 0, close > 0
    const auto status_at = [&](int z, int x) {
      const unsigned s = sget(L, z * nx + x);
      return s == kSKnown ? 0 : s == kSClose ? 1 : -1;
    };
    L->dec[k] = (signed char)handover_class(status_at, i, j, nz, nx);
  }
}

AF_DEV void clear_state(Lds* L, int nst, int tid) {
  for (int k = tid; k < (nst + 15) / 16; k += kThreads) L->st[k] = 0u;
  for (int k = tid; k < kHT; k += kThreads) L->ht[k] = 0u;
  if (tid == 0) L->nused = 0;
}

AF_DEV void clear_grid(double* T, long n, int tid) {
  const double nan = __builtin_nan("");
  for (long k = tid; k < n; k += kThreads) gst(T + k, nan);
}

// wave 0: the hand-over from the previous grid s (classes in Lds::dec, T in HBM) into g, in
// row-major order: T copied, known nodes known, outer-known and close nodes into the heap (add,
// not fresh).  Chunks of 64 nodes: one memory round trip for the chunk's T, then lane 0 adds its
// heap nodes in order.
AF_DEV void handover(Lds* L, Heap& h, const double* sT, int snz, int snx, int isz_s, int isx_s, const XG& g, int isz_d,
                     int isx_d, int lane) {
  const int dz = (snz - 1) / 3 + 1, dx = (snx - 1) / 3 + 1, n = dz * dx;
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    int cls = 0, c = 0;
    double t = 0.0;
    if (k < n) {
      const int i = 3 * (k / dx), j = 3 * (k % dx);
      const int pz = isz_d + (i - isz_s) / 3, px = isx_d + (j - isx_s) / 3;
      cls = L->dec[k];
      t = gld(sT + (long)i * snx + j);
      gst(g.T + (long)pz * g.nx + px, t);
      c = g.loc(pz, px);
      if (cls == 1 || cls == 2) sset(L, c, kSKnown);
    }
    unsigned long long am = __ballot(k < n && cls >= 2);
    while (am) {
      const int l = __ffsll((long long)am) - 1;
      am &= am - 1;
      const int cl = __shfl(c, l);
      const double tl = lane_d(t, l);
      if (lane == 0) h.add(cl, tl, false);
    }
  }
}

// wave 0: heap adds of T's nodes (z0 + k dz, x0 + k dx), k < n, in order, keys from T (64 loads
// per round trip)
AF_DEV void add_run(Lds* L, Heap& h, const XG& g, int z0, int x0, int dz, int dx, int n, int lane) {
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    double t = 0.0;
    if (k < n) t = gld(g.T + (long)(z0 + k * dz) * g.nx + (x0 + k * dx));
    const int m = min(64, n - k0);
    for (int l = 0; l < m; l++) {
      const double tl = lane_d(t, l);
      const int z = z0 + (k0 + l) * dz, x = x0 + (k0 + l) * dx;
      if (lane == 0) h.add(g.loc(z, x), tl, false);
    }
  }
}

__global__ __launch_bounds__(kThreads) void fmm_exact_lds_kernel(BandParams P) {
  __shared__ Lds lds;
  Lds* L = &lds;
  const int src = blockIdx.x;
  crm::lds_init();
  if (src >= P.nsrc) return;
  BandSrc* B = P.src + src;
  const int tid = threadIdx.x, lane = tid & 63;
  const bool w0 = tid < 64;
  const DevModel& M = P.M;
  const int sg = P.sg, sgside = (sg - 1) / 2;
  const long isx = (long)sg * (long)rint((P.scx[src] - P.gox) / P.dnx);
  const long isz = (long)sg * (long)rint((P.scz[src] - P.goz) / P.dnz);
  const int nnz = P.nz, nnx = P.nx;
  __shared__ int err_s, ntr_s;
  if (tid == 0) err_s = 0;
  Heap h{L};
  Spec sp;
  sp.c = -1;
  sp.v = 0.0;
  sp.dirty = false;
  sp.vm = 0u;
  const double* pT = nullptr;
  int pnz = 0, pnx = 0, pisz = 0, pisx = 0;
  const int scales[2] = {9, 3};
  const int size1 = 2 * sg + (sg - 1) / 2, size2 = size1 + 3 * sg;
  for (int stg = 0; stg < 2; stg++) {
    __syncthreads();
    if (err_s) break;
    const int scale = scales[stg], size = stg == 0 ? size1 : size2;
    const int left = (int)max(0L, isx - size), right = (int)min((long)nnx - 1, isx + size);
    const int bottom = (int)max(0L, isz - size), top = (int)min((long)nnz - 1, isz + size);
    XG g;
    g.nz = scale * (top - bottom) + 1;
    g.nx = scale * (right - left) + 1;
    g.wz0 = g.wx0 = 0;
    g.wh = g.nz;
    g.ww = g.nx;
    if ((long)g.nz * g.nx > P.capS || (long)g.nz * g.nx > kCap) {
      if (tid == 0) err_s = 9;
      break;
    }
    g.T = gptr(B->Ts[stg]);
    g.mv = MatView{scale, (scale - 1) / 2, bottom, scale, (scale - 1) / 2, left, sg, sgside, 0, 0, 1};
    g.dnx = g.dnz = P.dnx / scale;
    const int isx_s = scale * (int)(isx - left), isz_s = scale * (int)(isz - bottom);
    if (stg == 1) classify(L, pnz, pnx, tid);  // the previous grid's statuses, before they are cleared
    __syncthreads();
    clear_state(L, g.nz * g.nx, tid);
    clear_grid(g.T, (long)g.nz * g.nx, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave's clear lands before wave 0 writes
    __syncthreads();
    h.ntr = 0;
    h.ndup = 0;
    h.s.livedup = 0;
    if (stg == 0) {
      // straight rays (:2223-2267; veln + angle, SURVEY B-D5), material of the source's fine cell
      const int side1 = (9 - 1) / 2 + 9 * ((sg - 1) / 2);
      const MatView fine{sg, sgside, 0, sg, sgside, 0, 1, 0, 0, 0, 1};
      const CellMat cs = cell_mat(M, fine, (int)isz, (int)isx);
      const int w = 2 * side1 + 1;
      for (int k = tid; k < w * w; k += kThreads) {
        const int i = k / w - side1, j = k % w - side1;
        if (0 <= isz_s + i && isz_s + i <= g.nz - 1 && 0 <= isx_s + j && isx_s + j <= g.nx - 1) {
          double angle = (j == 0) ? 90.0 : AF_ATAN((double)i / (double)j) * kRad2Deg;
          double eff = pymod(cs.veln + angle, 180);
          double velocity = (cs.velpn != 0 || cs.stif == nullptr) ? table_vel(M.gtab, M.ncol, eff, cs.velpn, cs.vm)
                                                                  : christoffel_group(cs.stif, eff, cs.vm);
          double length = g.dnx * sqrt((double)(i * i + j * j));
          gst(g.T + (long)(isz_s + i) * g.nx + isx_s + j, length / velocity);
          sset(L, (isz_s + i) * g.nx + isx_s + j, kSKnown);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (w0) {
        // window edges -> heap in the reference's order (:2277-2288)
        const int s1 = side1;
        const int xa = max(0, isx_s - s1), xb = min(g.nx - 1, isx_s + s1);
        const int za = max(0, isz_s - s1), zb = min(g.nz - 1, isz_s + s1);
        if (isz_s - s1 >= 0) add_run(L, h, g, isz_s - s1, xa, 0, 1, xb - xa + 1, lane);
        if (isz_s + s1 <= g.nz - 1) add_run(L, h, g, isz_s + s1, xa, 0, 1, xb - xa + 1, lane);
        if (isx_s - s1 >= 0) add_run(L, h, g, za, isx_s - s1, 1, 0, zb - za + 1, lane);
        if (isx_s + s1 <= g.nx - 1) add_run(L, h, g, za, isx_s + s1, 1, 0, zb - za + 1, lane);
      }
    } else if (w0) {
      handover(L, h, pT, pnz, pnx, pisz, pisx, g, isz_s, isx_s, lane);
    }
    if (tid == 0) {
      L->cmd = 0;
      L->done = 0;
      L->applied = 0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // wave 0's grid stores before wave 1 reads them
    __syncthreads();
    if (w0) {
      const long long pops = heap_role(L, h, g, true, isx_s, isz_s, scale * size, 0.0, lane, B->ph);
      if (lane == 0) {
        B->steps[stg] = pops;
        if (h.err) err_s = h.err;
      }
    } else if (tid < 128) {
      relax_role(L, M, g, sp, lane, B->sub, B->ph);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    pT = g.T;
    pnz = g.nz;
    pnx = g.nx;
    pisz = isz_s;
    pisx = isx_s;
  }
  __syncthreads();
  // fine main grid (memset by the host: T NaN, S -1): the statuses of a window around the source
  // that holds the stage-2 hand-over and the prefix out to tstop
  const int Wh = size2 + P.exact_r + 8;  // tstop = (size2 + exact_r) dnx / vmax
  XG g;
  g.T = gptr(B->T);
  g.nz = nnz;
  g.nx = nnx;
  g.wz0 = (int)max(0L, isz - Wh);
  g.wx0 = (int)max(0L, isx - Wh);
  g.wh = (int)min((long)nnz - 1, isz + Wh) - g.wz0 + 1;
  g.ww = (int)min((long)nnx - 1, isx + Wh) - g.wx0 + 1;
  g.mv = MatView{sg, sgside, 0, sg, sgside, 0, 1, 0, 0, 0, 1};
  g.dnx = P.dnx;  // the coarse spacing on the fine grid (:2790; field divided by sg at the end)
  g.dnz = P.dnz;
  if (!err_s && (long)g.wh * g.ww > kCap && tid == 0) err_s = 9;
  if (!err_s) classify(L, pnz, pnx, tid);
  __syncthreads();
  int err = err_s;
  if (!err) {
    clear_state(L, g.wh * g.ww, tid);
    __syncthreads();
    if (w0) {
      h.ntr = 0;
      h.ndup = 0;
      h.s.livedup = 0;
      handover(L, h, pT, pnz, pnx, pisz, pisx, g, (int)isz, (int)isx, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (tid == 0) {
      L->cmd = 0;
      L->done = 0;
      L->applied = 0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // wave 0's grid stores before wave 1 reads them
    __syncthreads();
    if (w0) {
      const long long pops = heap_role(L, h, g, false, 0, 0, 0, P.tstop, lane, B->ph);
      if (lane == 0) {
        B->steps[2] = pops;
        if (h.err) err_s = h.err;
      }
    } else if (tid < 128) {
      relax_role(L, M, g, sp, lane, B->sub, B->ph);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    err = err_s;
  }
  // outputs for the band kernel: the window as the written box, known nodes' status 0 in S,
  // close nodes (heap entries) -> S = heap index, Lin
  if (!err) {
    const int n = g.wh * g.ww;
    for (int k = tid; k < n; k += kThreads)
      if (sget(L, k) == kSKnown) gst(B->S + (long)g.gz(k) * nnx + g.gx(k), (int)kKnown);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) ntr_s = h.ntr;
    __syncthreads();
    const int nl = ntr_s;
    for (int k = 1 + tid; k <= nl && k <= P.capL; k += kThreads) {
      const unsigned e = L->ent[k];
      const int c = (int)(e & kNodeM);
      const int f = g.gz(c) * nnx + g.gx(c);
      if (!(e & kDupF)) gst(B->S + f, k);  // close: 1 + close-list slot
      gst(B->Lin + k - 1, f);
    }
    // a node with two entries: its S is the later entry's index, as fmm_exact.hip's in-order loop
    if (tid == 0 && h.ndup) {
      for (int k = 1; k <= nl && k <= P.capL; k++) {
        const unsigned e = L->ent[k];
        if (e & kDupF) gst(B->S + g.gz(e & kNodeM) * nnx + g.gx(e & kNodeM), k);
      }
    }
    if (tid == 0) {
      B->bbox[0] = g.wz0;
      B->bbox[1] = g.wz0 + g.wh - 1;
      B->bbox[2] = g.wx0;
      B->bbox[3] = g.wx0 + g.ww - 1;
      B->nl0 = nl;
      if (nl > P.capL) err = 2;
    }
  }
  if (tid == 0) B->err = err;
}

}  // namespace xl
}  // namespace af

// 1: the LDS walk holds subgrid sg's stage grids and the prefix window (else fmm_exact.hip)
extern "C" int af_exact_lds_fits(int sg, int exact_r) {
  const long size1 = 2L * sg + (sg - 1) / 2, size2 = size1 + 3L * sg;
  const long s1 = 9 * 2 * size1 + 1, s2 = 3 * 2 * size2 + 1, w = 2 * (size2 + exact_r + 8) + 1;
  const long d1 = (s1 - 1) / 3 + 1, d2 = (s2 - 1) / 3 + 1;
  return s1 * s1 <= af::xl::kCap && s2 * s2 <= af::xl::kCap && w * w <= af::xl::kCap && d1 * d1 <= af::xl::kDec &&
         d2 * d2 <= af::xl::kDec;
}

extern "C" hipError_t af_launch_exact_lds(const af::BandParams* P, hipStream_t stream) {
  hipLaunchKernelGGL(af::xl::fmm_exact_lds_kernel, dim3(P->nsrc), dim3(af::xl::kThreads), 0, stream, *P);
  return hipGetLastError();
}
