// Sampled attribution over groups of columns (lsspa_set_players), host side.  Host-only C++: host_perms.cpp, which
// defines the two functions, is compiled without the HIP headers, and kernels.h includes this file for everyone else.
//
// PlayerMap is the map: labels [p] in {-1, 0 .. g-1} as a CSR -- group k owns cols[off[k] .. off[k+1]), ascending column
// index -- and the baseline's columns.  player_map_build returns nullptr, or what is wrong with the labels;
// expand_group_row writes the column ordering of one ordering of the groups (gperm [g], validated by the caller): the
// baseline, then the groups' columns in the order of gperm (read backwards when reversed != 0), each group's columns
// ascending.
#pragma once
#include <cstdint>
#include <vector>

namespace lsspa {

struct PlayerMap {
  int p = 0, g = 0;
  std::vector<int32_t> off, cols, base;
};
const char* player_map_build(const int32_t* labels, int p, int g, PlayerMap& m);
void expand_group_row(const PlayerMap& m, const int32_t* gperm, int reversed, int32_t* out);

// Sampled pairwise interactions (lsspa_pairs_batch): the three orderings of every sample.  perms [B][d] (validated by
// the caller) -> out [3 B][d]: row 3 s is perms[s], row 3 s + 1 perms[s] with positions (0,1), (2,3), .. swapped, row
// 3 s + 2 with positions (1,2), (3,4), .. swapped (a last position without a partner stays).
void expand_pair_rows(const int32_t* perms, int B, int d, int32_t* out);

}  // namespace lsspa
