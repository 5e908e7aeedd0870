// cr_levels_check — CPU test of the cyclic reduction's level arithmetic
// (cr_levels / cr_back_block, sqlm_plan.h: what launch_cr_core sizes its
// launches with) against a brute-force elimination, for p = 1 .. 600 in both
// numberings (lo = 0: first superblock at index 0, lo = 1: at index 1):
//   * every real superblock is eliminated exactly once or is the top;
//   * the existing neighbours I - h, I + h of an eliminated superblock are
//     alive at its level and survive it;
//   * ceil(log2 p) levels for lo = 0, floor(log2 p) for lo = 1;
//   * the grids (n_odd, n_even, back_grid) match the simulated counts and the
//     kernels' index maps (I = h + 2 h q, J = 2 h (q + lo)) enumerate them;
//   * k_cr_back_all's block -> (h, I) map, restated here as the kernel
//     computes it: every wait targets a lower workgroup id, or the top.
// Host only: neither HIP nor libsqrtlm.so. Prints one summary line; exit 0 = pass.
#include <cstdio>
#include <vector>

#include "../sqrtlm-slam_amd/csrc/sqlm_plan.h"

static int g_fail = 0;
#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c)) {                                         \
      if (g_fail < 20) {                                \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                       \
        std::printf("\n");                              \
      }                                                 \
      ++g_fail;                                         \
    }                                                   \
  } while (0)

// k_cr_back_all's loop, word for word: block b -> (h, I), coarsest level h_top first
static void device_back_map(int p, int lo, int h_top, int b, int &h, int &I) {
  h = h_top;
  for (;;) {
    const int n_odd = (p + lo - 1 + h) / (2 * h);
    if (b < n_odd || h == 1) break;
    b -= n_odd;
    h >>= 1;
  }
  I = h + 2 * h * b;
}

static void check(int p, int lo) {
  const sqlm::CRLevels L = sqlm::cr_levels(p, lo);
  const int first = lo, end = p + lo;  // real superblocks [first, end)
  std::vector<char> alive(end + 1, 0);
  std::vector<int> level_of(end + 1, -1);
  for (int I = first; I < end; ++I) alive[I] = 1;
  int want = 0;  // ceil(log2 p) or floor(log2 p)
  if (lo == 0) while ((1 << want) < p) ++want;
  else while ((2 << want) <= p) ++want;
  CHECK(L.count == want, "p %d lo %d: %d levels, expected %d", p, lo, L.count, want);
  CHECK(L.lo == lo, "p %d lo %d: lo field", p, lo);
  int eliminated = 0;
  for (int l = 0; l < L.count; ++l) {
    const int h = L.h[l];
    CHECK(h == 1 << l, "p %d lo %d level %d: h %d", p, lo, l, h);
    // brute force: the alive superblocks that are odd multiples of h go
    std::vector<int> odd, even;
    for (int I = first; I < end; ++I)
      if (alive[I]) {
        CHECK(I % h == 0, "p %d lo %d level %d: alive %d is no multiple of h", p, lo, l, I);
        ((I / h) % 2 ? odd : even).push_back(I);
      }
    CHECK((int)odd.size() + (int)even.size() >= 2, "p %d lo %d level %d runs on one superblock", p, lo, l);
    CHECK((int)odd.size() == L.n_odd[l], "p %d lo %d level %d: n_odd %d, simulated %zu", p, lo, l, L.n_odd[l], odd.size());
    CHECK((int)even.size() == L.n_even[l], "p %d lo %d level %d: n_even %d, simulated %zu", p, lo, l, L.n_even[l], even.size());
    for (int q = 0; q < (int)odd.size() && q < L.n_odd[l]; ++q)
      CHECK(odd[q] == h + 2 * h * q, "p %d lo %d level %d: odd %d is %d", p, lo, l, q, odd[q]);
    for (int q = 0; q < (int)even.size() && q < L.n_even[l]; ++q)
      CHECK(even[q] == 2 * h * (q + lo), "p %d lo %d level %d: even %d is %d", p, lo, l, q, even[q]);
    for (int I : odd) {
      for (int nb : {I - h, I + h})
        if (nb >= first && nb < end)
          CHECK(alive[nb] && (nb / h) % 2 == 0, "p %d lo %d level %d: neighbour %d of %d is gone or goes", p, lo, l, nb, I);
      CHECK((I - h >= first) || (I + h < end), "p %d lo %d level %d: %d has no neighbour", p, lo, l, I);
    }
    for (int I : odd) {
      CHECK(level_of[I] < 0, "p %d lo %d: %d eliminated twice", p, lo, I);
      alive[I] = 0;
      level_of[I] = l;
      ++eliminated;
    }
  }
  int left = 0, last = -1;
  for (int I = first; I < end; ++I)
    if (alive[I]) { ++left; last = I; }
  CHECK(left == 1 && last == L.top, "p %d lo %d: %d survivors, last %d, top %d", p, lo, left, last, L.top);
  CHECK(eliminated == p - 1 && L.back_grid == p - 1, "p %d lo %d: eliminated %d back_grid %d", p, lo, eliminated, L.back_grid);
  if (lo == 1) {
    CHECK((L.top & (L.top - 1)) == 0 && L.top <= p && 2 * L.top > p, "p %d: top %d", p, L.top);
  } else {
    CHECK(L.top == 0, "p %d: top %d", p, L.top);
  }
  // the one-launch back substitution: workgroup ids, and whom each waits for
  if (L.count == 0) return;
  std::vector<int> wg(end + 1, -1);
  for (int b = 0; b < L.back_grid; ++b) {
    int l, I, hd, Id;
    sqlm::cr_back_block(L, b, l, I);
    device_back_map(p, lo, L.h[L.count - 1], b, hd, Id);
    CHECK(hd == L.h[l] && Id == I, "p %d lo %d block %d: kernel map (%d, %d), host map (%d, %d)", p, lo, b, hd, Id, L.h[l], I);
    CHECK(I >= first && I < end && level_of[I] == l, "p %d lo %d block %d: (%d, %d) is not eliminated there", p, lo, b, L.h[l], I);
    if (I < first || I >= end) continue;
    CHECK(wg[I] < 0, "p %d lo %d: superblock %d has two workgroups", p, lo, I);
    wg[I] = b;
  }
  for (int I = first; I < end; ++I) {
    if (I == L.top) continue;
    CHECK(wg[I] >= 0, "p %d lo %d: superblock %d has no workgroup", p, lo, I);
    const int h = L.h[level_of[I] < 0 ? 0 : level_of[I]];
    for (int nb : {I - h, I + h})
      if (nb >= first && nb < end && nb != L.top)
        CHECK(wg[nb] >= 0 && wg[nb] < wg[I], "p %d lo %d: workgroup %d (I %d) waits for %d (I %d)", p, lo, wg[I], I, wg[nb], nb);
  }
}

int main() {
  int cases = 0;
  for (int lo = 0; lo <= 1; ++lo)
    for (int p = 1; p <= 600; ++p, ++cases) check(p, lo);
  std::printf("{\"cr_levels_check\": {\"cases\": %d, \"failures\": %d}}\n", cases, g_fail);
  return g_fail ? 1 : 0;
}
