// walk_heap.h — the reference's heap (addtree / updtree / downtree, Anis_TTF_rays.py:94-237), once,
// for the three exact walks (fmm_init.hip, fmm_exact.hip, fmm_exact_lds.hip).
//
// The heap decides the field near every source, so its quirks are kept exactly: the parent index
// is round(t / 2) half-even (:123, SURVEY B-D3), sifts move on strict '<' / '>', and heap indices
// are written in the reference's order (per level the moving entry's first, then the displaced
// one's; before a downtree the last entry's index is set to 1).  Keys are stored next to the
// entries (copies of the nodes' ttn), so a level costs one read of the other entry and key while
// the moving entry stays in registers.  The reference compares live ttn: a node with two heap
// entries (the stage-1 window corners, added by two of the edge loops) is recorded (dup list) and
// every key of its entries follows its ttn (sync).
//
// Where an entry's heap index is written is the store's business:
//   WalkStatusStore  the node's status word holds the index (nsts > 0), as in the reference;
//   WalkHashStore    a node -> index hash beside 2-bit status codes (far / close / known).
// A store gives: Entry; rd(pos, e, k) and rd2(pos, e1, k1, e2, k2) (slots pos, pos + 1) as single
// calls returning entries and keys; wr(pos, e, k); setpos(e, pos); node(e); in_heap(node);
// enter(node, pos, fresh, second, again) -> the new entry; dup(k) / set_dup(k, node);
// may_have_two(e): false only where the entry itself shows that its node has no other entry.
//
// Shared verbatim by the kernels and by a stand-alone host program (tests/walk_heap_sim.cpp, built
// with ASan and UBSan).  Includes nothing from HIP; the includer defines AF_DEV.
#pragma once

namespace af {

// round(t / 2), half-even, in integer arithmetic
AF_DEV int walk_parent(int t) {
  const int m = t >> 1;
  return (t & 1) ? m + (m & 1) : m;
}

// kCap heap slots (1-based: kCap - 1 entries), kDupCap nodes with two entries; err = kErr when
// either is exceeded: the refused add leaves the heap as it was.
template <class Store, int kCap, int kDupCap, int kErr>
struct WalkHeap {
  using Entry = typename Store::Entry;
  Store s;
  int ntr = 0, err = 0, ndup = 0;

  // entry em with key km rises from slot tpc (the tail of addtree and updtree)
  AF_DEV void sift_up(int tpc, Entry em, double km) {
    int tpp = walk_parent(tpc);
    while (tpp > 0) {
      Entry ep;
      double kp;
      s.rd(tpp, ep, kp);
      if (!(km < kp)) break;
      s.setpos(em, tpp);
      s.setpos(ep, tpc);
      s.wr(tpc, ep, kp);
      tpc = tpp;
      tpp = walk_parent(tpc);
    }
    s.wr(tpc, em, km);
  }
  AF_DEV bool is_dup(int node) const {
    bool d = false;
    for (int k = 0; k < ndup; k++) d |= s.dup(k) == node;
    return d;
  }
  // addtree :94-138.  key: the node's ttn; fresh: the node is known to be far, else its status
  // tells whether it already has an entry (then this is its second)
  AF_DEV void add(int node, double key, bool fresh) {
    ntr += 1;
    if (ntr >= kCap) {
      err = kErr;
      ntr = kCap - 1;
      return;
    }
    const bool second = !fresh && s.in_heap(node);
    if (second) {
      if (ndup == kDupCap) {
        err = kErr;
        ntr -= 1;
        return;
      }
      s.set_dup(ndup++, node);
    }
    const Entry e = s.enter(node, ntr, fresh, second, !fresh && !second && is_dup(node));
    s.setpos(e, ntr);
    sift_up(ntr, e, key);
  }
  // the ttn of entry e's node is key now: if the node has two entries, the keys of both follow
  AF_DEV void sync(Entry e, double key) {
    const int node = s.node(e);
    if (!s.may_have_two(e) || !is_dup(node)) return;
    for (int k = 1; k <= ntr; k++) {
      Entry ek;
      double ko;
      s.rd(k, ek, ko);
      if (s.node(ek) == node) s.wr(k, ek, key);
    }
  }
  // updtree :141-175: entry e at slot tpc (its node's heap index) has the lower key now.  The
  // node's other entry takes the key first: the reference's comparisons read the live ttn, so the
  // sift stops below that entry where it is an ancestor
  AF_DEV void upd(int tpc, Entry e, double key) {
    sync(e, key);
    sift_up(tpc, e, key);
  }
  // downtree :178-237
  AF_DEV void pop_down() {
    if (ntr == 1) {
      ntr = 0;
      return;
    }
    Entry em;
    double km;
    s.rd(ntr, em, km);
    s.setpos(em, 1);
    ntr -= 1;
    int tpp = 1, tpc = 2;
    while (tpc < ntr) {
      Entry e1, e2;
      double k1, k2;
      s.rd2(tpc, e1, k1, e2, k2);
      const bool right = k1 > k2;
      const int t = right ? tpc + 1 : tpc;
      const double kc = right ? k2 : k1;
      const Entry ec = right ? e2 : e1;
      if (kc < km) {
        s.setpos(em, t);
        s.setpos(ec, tpp);
        s.wr(tpp, ec, kc);
        tpp = t;
        tpc = 2 * tpp;
      } else {
        tpc = ntr + 1;
      }
    }
    if (tpc == ntr) {  // the last entry has no sibling
      Entry ec;
      double kc;
      s.rd(tpc, ec, kc);
      if (kc < km) {
        s.setpos(em, tpc);
        s.setpos(ec, tpp);
        s.wr(tpp, ec, kc);
        tpp = tpc;
      }
    }
    s.wr(tpp, em, km);
  }
};

// cell -> offset of its status word
struct WalkFlatMap {  // the cell is the offset
  AF_DEV int operator()(int c) const { return c; }
};
struct WalkPackedMap {  // cell z << 8 | x, rows of nx words
  int nx;
  AF_DEV int operator()(int c) const { return (c >> 8) * nx + (c & 255); }
};

// "The status word holds the index": entries are cells, S[map(cell)] > 0 is the heap index
// (0 known, -1 far).  Mem has key[], cell[] (heap slots) and dup[].
template <class Mem, class EntryT, class Word, class Map>
struct WalkStatusStore {
  using Entry = EntryT;
  Mem* m;
  Word* S;
  Map map;
  AF_DEV void rd(int pos, Entry& e, double& k) const {
    k = m->key[pos];
    e = m->cell[pos];
  }
  AF_DEV void rd2(int pos, Entry& e1, double& k1, Entry& e2, double& k2) const {
    k1 = m->key[pos];
    k2 = m->key[pos + 1];
    e1 = m->cell[pos];
    e2 = m->cell[pos + 1];
  }
  AF_DEV void wr(int pos, Entry e, double k) {
    m->cell[pos] = e;
    m->key[pos] = k;
  }
  AF_DEV void setpos(Entry e, int pos) { S[map((int)e)] = (Word)pos; }
  AF_DEV int node(Entry e) const { return (int)e; }
  AF_DEV bool in_heap(int node) const { return S[map(node)] > 0; }
  AF_DEV Entry enter(int node, int, bool, bool, bool) { return (Entry)node; }
  AF_DEV bool may_have_two(Entry) const { return true; }
  AF_DEV int dup(int k) const { return (int)m->dup[k]; }
  AF_DEV void set_dup(int k, int node) { m->dup[k] = (EntryT)node; }
};

// Heap indices in a hash (open addressing, 1 << kHTLog words: live | index << 18 | node; 0 empty,
// kTomb a freed slot) beside 2-bit status codes.  An entry is node | hash slot << 18 | kDupF, so a
// heap-index write is one store through the entry's slot; an entry of a node with two entries
// (kDupF) also makes the node close again, as the reference's nsts = index does after the node was
// popped through its other entry, and such a node keeps its slot when popped.  Mem has key[], ent[]
// (heap slots), ht[], nused (slots live or freed) and dup[].  Dev supplies the status codes'
// get(node) / set(node, code) (lanes share words on the device) and pin(e...), which may keep an
// entry's read next to its key's.  Nodes < 1 << 18, heap indices < 1 << 12, kHTLog <= 13.
constexpr unsigned kWalkFar = 0, kWalkClose = 1, kWalkKnown = 2;
template <class Mem, class Dev, int kHTLog>
struct WalkHashStore {
  using Entry = unsigned;
  static constexpr int kHT = 1 << kHTLog;
  static constexpr unsigned kLive = 1u << 30, kTomb = 0x80000000u, kNodeM = (1u << 18) - 1, kDupF = 0x80000000u;
  Mem* m;
  Dev dev;
  int livedup = 0;  // heap entries carrying kDupF
  AF_DEV static unsigned hslot(int c) { return ((unsigned)c * 2654435761u) >> (32 - kHTLog); }
  AF_DEV int hfind(int c) const {
    unsigned q = hslot(c);
    for (int p = 0; p < kHT; p++) {
      const unsigned w = m->ht[q];
      if (w == 0u) return -1;
      if ((w >> 30) == 1u && (int)(w & kNodeM) == c) return (int)q;
      q = (q + 1) & (kHT - 1);
    }
    return -1;
  }
  AF_DEV int hinsert(int c) {
    unsigned q = hslot(c);
    while (true) {
      const unsigned w = m->ht[q];
      if (w == 0u || w == kTomb) {
        if (w == 0u) m->nused++;
        m->ht[q] = kLive | (unsigned)c;
        return (int)q;
      }
      q = (q + 1) & (kHT - 1);
    }
  }
  AF_DEV int pos_of(int c) const { return (int)((m->ht[hfind(c)] >> 18) & 0xfffu); }
  AF_DEV void rd(int pos, Entry& e, double& k) const {
    k = m->key[pos];
    e = m->ent[pos];
    dev.pin(e);
  }
  AF_DEV void rd2(int pos, Entry& e1, double& k1, Entry& e2, double& k2) const {
    k1 = m->key[pos];
    k2 = m->key[pos + 1];
    e1 = m->ent[pos];
    e2 = m->ent[pos + 1];
    dev.pin(e1, e2);
  }
  AF_DEV void wr(int pos, Entry e, double k) {
    m->ent[pos] = e;
    m->key[pos] = k;
  }
  AF_DEV void setpos(Entry e, int pos) {
    m->ht[(e >> 18) & (kHT - 1)] = kLive | ((unsigned)pos << 18) | (e & kNodeM);
    if (e & kDupF) dev.set((int)(e & kNodeM), kWalkClose);
  }
  AF_DEV int node(Entry e) const { return (int)(e & kNodeM); }
  AF_DEV bool in_heap(int node) const { return dev.get(node) == kWalkClose; }
  // pos: the new entry's slot (the heap's last); again: the node had two entries before
  AF_DEV Entry enter(int c, int pos, bool fresh, bool second, bool again) {
    Entry e;
    if (second) {
      const int hs = hfind(c);
      for (int k = 1; k < pos; k++)  // its other entry now carries the flag
        if ((int)(m->ent[k] & kNodeM) == c && !(m->ent[k] & kDupF)) {
          m->ent[k] |= kDupF;
          livedup++;
        }
      e = (unsigned)c | ((unsigned)hs << 18) | kDupF;
    } else {
      int hs = fresh ? -1 : hfind(c);  // a popped node with two entries keeps its slot
      if (hs < 0) hs = hinsert(c);
      e = (unsigned)c | ((unsigned)hs << 18) | (again ? kDupF : 0u);
      dev.set(c, kWalkClose);
    }
    if (e & kDupF) livedup++;
    return e;
  }
  // the root entry e0 is popped: its hash slot is freed unless its node has another entry
  AF_DEV void leave(Entry e0) {
    if (!(e0 & kDupF)) m->ht[(e0 >> 18) & (kHT - 1)] = kTomb;
    else livedup--;
  }
  AF_DEV bool may_have_two(Entry e) const { return (e & kDupF) != 0u; }
  AF_DEV int dup(int k) const { return m->dup[k]; }
  AF_DEV void set_dup(int k, int node) { m->dup[k] = node; }
};

}  // namespace af
