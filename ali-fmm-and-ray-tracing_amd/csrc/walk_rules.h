// walk_rules.h — the small rules of the reference's heap walk that the three exact walks
// (fmm_init.hip, fmm_exact.hip, fmm_exact_lds.hip) share, each spelled once.  Like walk_heap.h:
// includes nothing from HIP, the includer defines AF_DEV, and tests/walk_heap_sim.cpp runs them on
// the host.
#pragma once

namespace af {

struct WalkNode {
  int z, x;
};

// neighbour k of a popped node in the reference's order: x - 1, x + 1, z - 1, z + 1.  Each is
// classified by its status: far -> addtree, close -> updtree, known -> skipped.
AF_DEV WalkNode walk_nbr(int k, int iz, int ix) {
  return WalkNode{k == 2 ? iz - 1 : k == 3 ? iz + 1 : iz, k == 0 ? ix - 1 : k == 1 ? ix + 1 : ix};
}
// the reference tests only the coordinate that neighbour k moved along
AF_DEV bool walk_in_grid(int k, WalkNode q, int nz, int nx) {
  return k < 2 ? (0 <= q.x && q.x <= nx - 1) : (0 <= q.z && q.z <= nz - 1);
}
// a stage walk ends with the pop that has an out-of-grid neighbour k at max_dist + 1 from the
// stage's source (isz, isx), along k's axis
AF_DEV bool walk_stage_stop(int k, WalkNode q, int isz, int isx, int max_dist) {
  const int d = k < 2 ? isx - q.x : isz - q.z;
  return (d < 0 ? -d : d) == max_dist + 1;
}

// the speculative relaxations' guesses: lane >= 1 evaluates neighbour dir of heap entry `entry`
// (the first 16 entries: the next pops)
struct WalkGuess {
  int entry, dir;
};
AF_DEV WalkGuess walk_guess(int lane) { return WalkGuess{1 + ((lane - 1) >> 2), (lane - 1) & 3}; }

// does the node at offset (dz, dx) lie in update()'s 12-point stencil (NbField's slots): the axis
// neighbours at distance 1 and 2 and the four diagonal ones, i.e. every node at |dz| + |dx| 1 or 2
AF_DEV bool stencil_holds(int dz, int dx) {
  const int ad = (dz < 0 ? -dz : dz) + (dx < 0 ? -dx : dx);
  return ad == 1 || ad == 2;
}

// hand-over class of node (i, j) of an nz x nx grid whose every third node goes to the next grid:
// 0 far, 1 known, 2 known with a far or missing node 3 away ("outer": it enters the next heap),
// 3 close.  status_at(i, j): -1 far, 0 known, > 0 close.
template <class StatusAt>
AF_DEV int handover_class(const StatusAt& status_at, int i, int j, int nz, int nx) {
  const int st = status_at(i, j);
  if (st > 0) return 3;
  if (st != 0) return 0;
  const bool outer = i - 3 < 0 || status_at(i - 3, j) == -1 || i + 3 > nz - 1 || status_at(i + 3, j) == -1 ||
                     j - 3 < 0 || status_at(i, j - 3) == -1 || j + 3 > nx - 1 || status_at(i, j + 3) == -1;
  return outer ? 2 : 1;
}

}  // namespace af
