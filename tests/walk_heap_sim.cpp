// walk_heap_sim.cpp — csrc/walk_heap.h and csrc/walk_rules.h on the host, under ASan and UBSan
// (tests/test_walk_heap.py builds and runs it).  The shared heap runs with each of its three
// stores (packed cells + short status words as fmm_init.hip, flat cells + int status words as
// fmm_exact.hip, the hash store as fmm_exact_lds.hip) beside a plain live-key heap on ttn / nsts /
// btg, restated here from oracle/alifmm_oracle.c's addtree / updtree / downtree; after every
// operation of seeded FMM-shaped sequences the heaps must agree slot by slot and node by node.
// Exits non-zero with a message on the first difference; prints the event counts on success.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <type_traits>
#include <vector>

#define AF_DEV inline
#include "walk_heap.h"
#include "walk_rules.h"

using namespace af;

#define CHECK(c, ...)                      \
  do {                                     \
    if (!(c)) {                            \
      std::printf("FAIL %s: ", #c);        \
      std::printf(__VA_ARGS__);            \
      std::printf("\n");                   \
      std::exit(1);                        \
    }                                      \
  } while (0)

// events the sequences must meet (counted on the model alone)
struct Events {
  long second_add = 0, sync_multi = 0, pop_first = 0, pop_second = 0, tail = 0, root = 0, err_full = 0, err_dup = 0;
};
static Events ev;

// ---- the model: the reference's heap, comparisons on the live ttn ----
struct Model {
  int n, ntr = 0;
  std::vector<double> ttn;
  std::vector<int> nsts, btg, popped;
  explicit Model(int n_) : n(n_), ttn(n_, 0.0), nsts(n_, -1), btg(n_ * 2 + 8, 0), popped(n_, 0) {}
  static int parent(int t) { return (int)std::rint(t / 2.0); }
  double tb(int k) const { return ttn[btg[k]]; }
  int entries(int c) const {
    int m = 0;
    for (int k = 1; k <= ntr; k++) m += btg[k] == c;
    return m;
  }
  void sift(int c, int tpc) {
    const int start = tpc;
    int tpp = parent(tpc);
    const double tv = ttn[c];
    while (tpp > 0) {
      if (tv < tb(tpp)) {
        nsts[c] = tpp;
        nsts[btg[tpp]] = tpc;
        std::swap(btg[tpc], btg[tpp]);
        tpc = tpp;
        tpp = parent(tpc);
      } else {
        tpp = 0;
      }
    }
    if (tpc == 1 && start != 1) ev.root++;
  }
  void addtree(int c) {
    if (nsts[c] > 0) ev.second_add++;
    ntr += 1;
    nsts[c] = ntr;
    btg[ntr] = c;
    sift(c, ntr);
  }
  void updtree(int c) {
    if (entries(c) > 1) ev.sync_multi++;
    sift(c, nsts[c]);
  }
  void pop() {  // the walk's pop: the root is known, then downtree
    const int c = btg[1];
    if (popped[c]) ev.pop_second++;
    else if (entries(c) > 1) ev.pop_first++;
    popped[c] = 1;
    nsts[c] = 0;
    if (ntr == 1) {
      ntr = 0;
      return;
    }
    nsts[btg[ntr]] = 1;
    btg[1] = btg[ntr];
    ntr -= 1;
    int tpp = 1, tpc = 2;
    while (tpc < ntr) {
      if (tb(tpc) > tb(tpc + 1)) tpc = tpc + 1;
      if (tb(tpc) < tb(tpp)) {
        nsts[btg[tpp]] = tpc;
        nsts[btg[tpc]] = tpp;
        std::swap(btg[tpc], btg[tpp]);
        tpp = tpc;
        tpc = 2 * tpp;
      } else {
        tpc = ntr + 1;
      }
    }
    if (tpc == ntr) {
      ev.tail++;
      if (tb(tpc) < tb(tpp)) {
        nsts[btg[tpp]] = tpc;
        nsts[btg[tpc]] = tpp;
        std::swap(btg[tpc], btg[tpp]);
      }
    }
  }
};

// ---- the shared heap behind one interface per store: flat nodes c = z * nx + x ----
template <int kCap, int kDupCap>
struct StatusMem {
  double key[kCap];
  int cell[kCap];
  int dup[kDupCap];
};
template <int kCap, int kDupCap>
struct PackedMem {
  double key[kCap];
  unsigned short cell[kCap];
  unsigned short dup[kDupCap];
};

// the status word holds the index; Packed: cells z << 8 | x and short words (fmm_init.hip), else
// flat cells and int words (fmm_exact.hip)
template <bool Packed, int kCap, int kDupCap>
struct StatusDriver {
  using Mem = typename std::conditional<Packed, PackedMem<kCap, kDupCap>, StatusMem<kCap, kDupCap>>::type;
  using Word = typename std::conditional<Packed, short, int>::type;
  using Ent = typename std::conditional<Packed, unsigned short, int>::type;
  using Map = typename std::conditional<Packed, WalkPackedMap, WalkFlatMap>::type;
  int nx;
  Mem* mem = new Mem();
  std::vector<Word> S;
  WalkHeap<WalkStatusStore<Mem, Ent, Word, Map>, kCap, kDupCap, 7> h;
  StatusDriver(int nz, int nx_) : nx(nx_), S(nz * nx_, (Word)-1) {
    h.s.m = mem;
    h.s.S = S.data();
    set_pitch(h.s.map, nx_);
  }
  ~StatusDriver() { delete mem; }
  static void set_pitch(WalkPackedMap& m, int nx) { m.nx = nx; }
  static void set_pitch(WalkFlatMap&, int) {}
  int enc(int c) const { return Packed ? ((c / nx) << 8) | (c % nx) : c; }
  int dec(int e) const { return Packed ? (e >> 8) * nx + (e & 255) : e; }
  void add(int c, double key, bool fresh) { h.add(enc(c), key, fresh); }
  void upd(int c, double key) {
    h.upd(S[c], (Ent)enc(c), key);
  }
  void pop() {
    S[dec(mem->cell[1])] = 0;
    h.pop_down();
  }
  int node_at(int k) const { return dec(mem->cell[k]); }
  double key_at(int k) const { return mem->key[k]; }
  void check_node(int c, int nsts) const { CHECK(S[c] == nsts, "node %d status %d, model %d", c, (int)S[c], nsts); }
};

// the hash store at the production table size (1 << 13), its 2-bit codes in a plain array
constexpr int kSimHTLog = 13;
template <int kCap, int kDupCap>
struct HashMem {
  double key[kCap];
  unsigned ent[kCap];
  unsigned ht[1 << kSimHTLog];
  int dup[kDupCap];
  int nused;
};
struct HashDev {
  std::vector<unsigned char>* st;
  unsigned get(int c) const { return (*st)[c]; }
  void set(int c, unsigned v) const { (*st)[c] = (unsigned char)v; }
  void pin(unsigned&) const {}
  void pin(unsigned&, unsigned&) const {}
};
template <int kCap, int kDupCap>
struct HashDriver {
  using Mem = HashMem<kCap, kDupCap>;
  Mem* mem = new Mem();
  std::vector<unsigned char> st;
  WalkHeap<WalkHashStore<Mem, HashDev, kSimHTLog>, kCap, kDupCap, 7> h;
  HashDriver(int nz, int nx) : st(nz * nx, (unsigned char)kWalkFar) {
    h.s.m = mem;
    h.s.dev.st = &st;
  }
  ~HashDriver() { delete mem; }
  void add(int c, double key, bool fresh) { h.add(c, key, fresh); }
  void upd(int c, double key) {
    const int pos = h.s.pos_of(c);
    h.upd(pos, mem->ent[pos], key);
  }
  void pop() {
    h.s.dev.set(h.s.node(mem->ent[1]), kWalkKnown);
    h.s.leave(mem->ent[1]);
    h.pop_down();
  }
  int node_at(int k) const { return h.s.node(mem->ent[k]); }
  double key_at(int k) const { return mem->key[k]; }
  void check_node(int c, int nsts) const {
    const unsigned want = nsts < 0 ? kWalkFar : nsts == 0 ? kWalkKnown : kWalkClose;
    CHECK(st[c] == want, "node %d code %u, model status %d", c, (unsigned)st[c], nsts);
    if (nsts > 0) CHECK(h.s.pos_of(c) == nsts, "node %d index %d, model %d", c, h.s.pos_of(c), nsts);
  }
};

template <class D>
static void compare(const Model& m, const D& d, long op) {
  CHECK(d.h.ntr == m.ntr && d.h.err == 0, "op %ld: ntr %d (model %d), err %d", op, d.h.ntr, m.ntr, d.h.err);
  for (int k = 1; k <= m.ntr; k++) {
    CHECK(d.node_at(k) == m.btg[k], "op %ld slot %d: node %d, model %d", op, k, d.node_at(k), m.btg[k]);
    CHECK(d.key_at(k) == m.tb(k), "op %ld slot %d: key %.17g, model's live ttn %.17g", op, k, d.key_at(k), m.tb(k));
  }
  for (int c = 0; c < m.n; c++) d.check_node(c, m.nsts[c]);
}

// One FMM-shaped sequence on an nz x nx grid, through the model and (D = a driver) the shared
// heap, compared after every operation; Model-only when D is void.  A front grows from a seed
// node: far neighbours of popped nodes are added, close ones lowered; some close nodes get a
// second entry (as the stage-1 window corners do), are lowered again and popped through both.
template <class D>
static void run_sequence(int nz, int nx, unsigned seed, int nops) {
  std::mt19937 rng(seed);
  auto rnd = [&](int n) { return (int)(rng() % (unsigned)n); };
  auto frac = [&]() { return (double)(rng() % 100000u) / 100000.0; };
  Model m(nz * nx);
  D d(nz, nx);
  // (the hash store: fewer distinct inserts than its rehash threshold; rehash() is the kernel's)
  CHECK(nz * nx < (3 << kSimHTLog) / 4, "%d x %d nodes", nz, nx);
  int seconds = 0;  // nodes given a second entry (the dup cap is 8)
  long op = 0;
  auto add = [&](int c, double t, bool fresh) {
    m.ttn[c] = t;
    m.addtree(c);
    d.add(c, t, fresh);
    compare(m, d, ++op);
  };
  auto lower = [&](int c, double t) {
    m.ttn[c] = t;
    m.updtree(c);
    d.upd(c, t);
    compare(m, d, ++op);
  };
  for (int k = 0; k < 6; k++) {  // the first front
    const int c = rnd(nz * nx);
    if (m.nsts[c] < 0) add(c, 1.0 + frac(), k & 1);
  }
  for (int it = 0; it < nops && m.ntr > 0; it++) {
    const int what = rnd(10);
    if (what < 5) {  // pop, then the walk's four neighbours
      const int c = m.btg[1];
      const double t0 = m.ttn[c];
      m.pop();
      d.pop();
      compare(m, d, ++op);
      for (int k = 0; k < 4; k++) {
        const WalkNode q = walk_nbr(k, c / nx, c % nx);
        if (q.z < 0 || q.z >= nz || q.x < 0 || q.x >= nx) continue;
        const int b = q.z * nx + q.x;
        if (m.nsts[b] < 0) add(b, t0 + 0.1 + frac(), rnd(2));
        else if (m.nsts[b] > 0 && rnd(2)) lower(b, m.ttn[b] - 0.3 * frac());
      }
    } else if (what < 7 && m.ntr < 400) {  // a far node anywhere
      const int c = rnd(nz * nx);
      if (m.nsts[c] < 0) add(c, m.tb(1) + 2.0 * frac(), rnd(2));
    } else if (what < 8) {  // a second entry for a close node that has one and was never popped
      const int c = m.btg[1 + rnd(m.ntr)];
      if (m.nsts[c] > 0 && m.entries(c) == 1 && !m.popped[c] && seconds < 8) {
        seconds++;
        add(c, m.ttn[c], false);
      }
    } else {  // lower a close node's key
      const int c = m.btg[1 + rnd(m.ntr)];
      if (m.nsts[c] > 0) lower(c, m.ttn[c] - 0.5 * frac());
    }
  }
  while (m.ntr > 0) {  // drain: every entry popped, second entries included
    m.pop();
    d.pop();
    compare(m, d, ++op);
  }
}

// a driver that runs nothing: the model alone (the seeds must produce every event by themselves)
struct ModelOnly {
  ModelOnly(int, int) {}
  void add(int, double, bool) {}
  void upd(int, double) {}
  void pop() {}
};
template <>
void compare<ModelOnly>(const Model&, const ModelOnly&, long) {}

struct Case {
  int nz, nx;
  unsigned seed;
  int nops;
};
static const Case kCases[] = {{9, 9, 11u, 400}, {16, 16, 5u, 900}, {7, 40, 23u, 900}, {16, 16, 77u, 900}};

// ---- error paths: 16 heap slots, 2 nodes with two entries; ASan judges every access ----
template <class D>
static void run_errors() {
  {  // the heap fills up: slots 1..15, the 16th add is refused
    D d(6, 6);
    for (int c = 0; c < 15; c++) d.add(c, 10.0 - c, false);
    CHECK(d.h.err == 0 && d.h.ntr == 15, "15 entries fit: err %d ntr %d", d.h.err, d.h.ntr);
    d.add(20, 0.5, false);
    CHECK(d.h.err == 7 && d.h.ntr == 15, "full heap: err %d ntr %d", d.h.err, d.h.ntr);
    ev.err_full++;
    d.add(21, 0.25, true);
    d.upd(3, -100.0);
    CHECK(d.node_at(1) == 3, "later operations still work: root %d", d.node_at(1));
    while (d.h.ntr > 0) d.pop();
  }
  {  // the third node with two entries is refused
    D d(6, 6);
    for (int c = 0; c < 6; c++) d.add(c, 1.0 + c, false);
    d.add(0, 1.0, false);
    d.add(1, 2.0, false);
    CHECK(d.h.err == 0 && d.h.ndup == 2 && d.h.ntr == 8, "two fit: err %d ndup %d", d.h.err, d.h.ndup);
    d.add(2, 3.0, false);
    CHECK(d.h.err == 7 && d.h.ndup == 2 && d.h.ntr == 8, "dup cap: err %d ndup %d ntr %d", d.h.err, d.h.ndup, d.h.ntr);
    ev.err_dup++;
    d.upd(1, 0.5);
    d.add(30, 0.1, true);
    while (d.h.ntr > 0) d.pop();
  }
}

int main() {
  // 1. the parent index
  for (int t = 1; t <= 1 << 20; t++)
    CHECK(walk_parent(t) == (int)std::rint(t / 2.0), "walk_parent(%d) = %d", t, walk_parent(t));

  // 2. the sequences: first the model alone, which must meet every event
  for (const Case& c : kCases) run_sequence<ModelOnly>(c.nz, c.nx, c.seed, c.nops);
  const Events alone = ev;
  CHECK(alone.second_add > 0 && alone.sync_multi > 0 && alone.pop_first > 0 && alone.pop_second > 0 &&
            alone.tail > 0 && alone.root > 0,
        "the model alone: second_add %ld sync_multi %ld pop_first %ld pop_second %ld tail %ld root %ld",
        alone.second_add, alone.sync_multi, alone.pop_first, alone.pop_second, alone.tail, alone.root);
  for (const Case& c : kCases) {
    run_sequence<StatusDriver<true, 1024, 8>>(c.nz, c.nx, c.seed, c.nops);
    run_sequence<StatusDriver<false, 8192, 8>>(c.nz, c.nx, c.seed, c.nops);
    run_sequence<HashDriver<4096, 8>>(c.nz, c.nx, c.seed, c.nops);
  }

  // 3. the error paths
  run_errors<StatusDriver<true, 16, 2>>();
  run_errors<StatusDriver<false, 16, 2>>();
  run_errors<HashDriver<16, 2>>();

  // 4. stencil_holds against NbField's 12 slots (fields.h: NbField::load's offsets)
  {
    const int sz[12] = {0, 0, 0, 0, -2, -1, 1, 2, -1, -1, 1, 1}, sx[12] = {-2, -1, 1, 2, 0, 0, 0, 0, -1, 1, -1, 1};
    for (int dz = -3; dz <= 3; dz++)
      for (int dx = -3; dx <= 3; dx++) {
        bool in = false;
        for (int k = 0; k < 12; k++) in |= sz[k] == dz && sx[k] == dx;
        CHECK(stencil_holds(dz, dx) == in, "stencil_holds(%d, %d)", dz, dx);
      }
  }

  // 5. handover_class on a 10 x 13 grid: '.' far, 'k' known, 'c' close; every third node classed
  {
    // far nodes 3 above (3,6), left of (3,3), right of (3,9) and below (6,3); (6,6) has only known
    // and close nodes around it; every other known node stands at an edge
    const char* g[10] = {"kkkkkk.kkkkkk", "kkkkkkkkkkkkk", "kkkkkkkkkkkkk", ".kkkkkkkkkkk.", "kkkkkkkkkkkkk",
                         "kkkkkkkkkkkkk", "kkkkkkkkkckkc", "kkkkkkkkkkkkk", "kkkkkkkkkkkkk", "kkk.kkkkkkkkk"};
    const int want[4][5] = {{2, 2, 0, 2, 2}, {0, 2, 2, 2, 0}, {2, 2, 1, 3, 3}, {2, 0, 2, 2, 2}};
    const auto status_at = [&](int z, int x) { return g[z][x] == '.' ? -1 : g[z][x] == 'k' ? 0 : 5; };
    for (int i = 0; i < 10; i += 3)
      for (int j = 0; j < 13; j += 3) {
        const int cls = handover_class(status_at, i, j, 10, 13);
        CHECK(cls == want[i / 3][j / 3], "handover_class(%d, %d) = %d, expected %d", i, j, cls, want[i / 3][j / 3]);
      }
  }

  // 6. the neighbour order, the stage stop and the guesses' placement
  {
    const int nz[4] = {5, 5, 4, 6}, nx[4] = {6, 8, 7, 7};
    for (int k = 0; k < 4; k++) {
      const WalkNode q = walk_nbr(k, 5, 7);
      CHECK(q.z == nz[k] && q.x == nx[k], "walk_nbr(%d) = (%d, %d)", k, q.z, q.x);
    }
    CHECK(!walk_in_grid(0, WalkNode{3, -1}, 9, 9) && walk_in_grid(1, WalkNode{3, 8}, 9, 9) &&
              !walk_in_grid(1, WalkNode{3, 9}, 9, 9) && !walk_in_grid(2, WalkNode{-1, 3}, 9, 9) &&
              !walk_in_grid(3, WalkNode{9, 3}, 9, 9) && walk_in_grid(2, WalkNode{0, 3}, 9, 9),
          "walk_in_grid");
    // a stage whose source is at (4, 4) with max_dist 4 on a 9 x 9 grid: the neighbours off each edge
    CHECK(walk_stage_stop(0, WalkNode{2, -1}, 4, 4, 4) && walk_stage_stop(1, WalkNode{2, 9}, 4, 4, 4) &&
              walk_stage_stop(2, WalkNode{-1, 7}, 4, 4, 4) && walk_stage_stop(3, WalkNode{9, 0}, 4, 4, 4) &&
              !walk_stage_stop(0, WalkNode{2, -1}, 4, 5, 4) && !walk_stage_stop(3, WalkNode{9, 0}, 3, 4, 4),
          "walk_stage_stop");
    const int ge[6] = {1, 1, 1, 1, 2, 16}, gd[6] = {0, 1, 2, 3, 0, 2}, gl[6] = {1, 2, 3, 4, 5, 63};
    for (int k = 0; k < 6; k++) {
      const WalkGuess w = walk_guess(gl[k]);
      CHECK(w.entry == ge[k] && w.dir == gd[k], "walk_guess(%d) = (%d, %d)", gl[k], w.entry, w.dir);
    }
  }

  std::printf("ok second_add=%ld sync_multi=%ld pop_first=%ld pop_second=%ld tail=%ld root=%ld err_full=%ld err_dup=%ld\n",
              alone.second_add, alone.sync_multi, alone.pop_first, alone.pop_second, alone.tail, alone.root,
              ev.err_full, ev.err_dup);
  return 0;
}
