// Sampled attribution over groups of columns (lsspa_set_players), host side.  Host-only C++: host_perms.cpp, which
// defines the two functions, is compiled without the HIP headers, and kernels.h includes this file for everyone else.
//
// PlayerMap is the map: labels [p] in {-1, 0 .. g-1} as a CSR -- group k owns cols[off[k] .. off[k+1]), ascending column
// index -- and the baseline's columns.  player_map_build returns nullptr, or what is wrong with the labels;
// expand_group_row writes the column ordering of one ordering of the groups (gperm [g], validated by the caller): the
// baseline, then the groups' columns in the order of gperm (read backwards when reversed != 0), each group's columns
// ascending.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lsspa {

struct PlayerMap {
  int p = 0, g = 0;
  std::vector<int32_t> off, cols, base;
};
const char* player_map_build(const int32_t* labels, int p, int g, PlayerMap& m);
void expand_group_row(const PlayerMap& m, const int32_t* gperm, int reversed, int32_t* out);

// The sampled families' host side (lsspa_multi_lift_*, lsspa_cv_lift_*, lsspa_boot_lift_*); each returns nullptr or the
// refusal's text, written into msg.
// The orderings of a call, perms [count][d] (d = g with a map, else p): not NULL, 1 <= count, limit_rows count p < 2^31
// (limit_rows: 1 or 2 rows of p a sample on the device), every row a permutation of 0 .. d-1.
const char* lift_orderings_why(const char* entry, const char* count_name, const int32_t* perms, int64_t count, int p, int g,
                               int d, int limit_rows, std::vector<int32_t>& mark, char* msg, size_t len);
// The rows of samples s0 .. s0 + ns - 1 as the device takes them: without a map (g == 0) the caller's own rows; with one,
// rows [ns][per][p] = the expansions of the samples' group orderings, the second of a pair reversed (rows grows to fit).
const int32_t* lift_stage_rows(const PlayerMap& m, int g, const int32_t* perms, int64_t s0, int64_t ns, int per, int p,
                               std::vector<int32_t>& rows);
// nf [K] = rows of every fold; labels outside 0 .. K-1 and an empty fold are refused.
const char* cv_count_folds(const int32_t* fold_ids, int64_t N, int K, int32_t* nf, char* msg, size_t len);

// Sampled pairwise interactions (lsspa_pairs_batch): the three orderings of every sample.  perms [B][d] (validated by
// the caller) -> out [3 B][d]: row 3 s is perms[s], row 3 s + 1 perms[s] with positions (0,1), (2,3), .. swapped, row
// 3 s + 2 with positions (1,2), (3,4), .. swapped (a last position without a partner stays).
void expand_pair_rows(const int32_t* perms, int B, int d, int32_t* out);

}  // namespace lsspa
