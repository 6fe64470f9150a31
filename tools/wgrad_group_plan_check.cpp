// CPU check of the grouped weight-gradient planner (csrc/wgrad_group_plan.hpp):
// replays the kernel's block -> (member, (o, c) tile, split) mapping on the
// host for a sweep of member mixes and asserts that
//   * every (member, o tile, c tile, pixel tile) is covered exactly once,
//   * every block index maps inside the tables and the block count is the grid,
//   * every pixel tile's use index is one of the member's use slots,
//   * the partial regions are 256-byte aligned, disjoint and inside the
//     reported workspace size.
// Build: c++ -std=c++17 -fsanitize=address,undefined -I dro-sfm_amd/csrc
//        tools/wgrad_group_plan_check.cpp   (tests/test_wgrad_group_plan.py)
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "wgrad_group_plan.hpp"

using namespace dro;

#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

static long long g_plans = 0;

static void check(const std::vector<WgGroupShape>& s, int KH, int KW, int target) {
  WgGroupPlan pl;
  const int n = (int)s.size(), T = KH * KW;
  CHECK(wgrad_group_plan(s.data(), n, KH, KW, target, &pl));
  ++g_plans;
  CHECK(pl.nmember == n);
  // the tables the kernel searches: first block of each member, INT_MAX past the last
  int block0[kGroupMembers], fin0[kGroupMembers];
  for (int i = 0; i < kGroupMembers; ++i) {
    block0[i] = i < n ? pl.m[i].block0 : INT_MAX;
    fin0[i] = i < n ? pl.m[i].fin0 : INT_MAX;
  }
  std::vector<std::vector<int>> cover(n);
  std::vector<std::pair<size_t, size_t>> regions;
  int blocks = 0, fin = 0, nuse = 0;
  for (int i = 0; i < n; ++i) {
    const WgGroupMemberPlan& m = pl.m[i];
    CHECK(m.block0 == blocks && m.fin0 == fin && m.use0 == nuse);
    CHECK(m.splits >= 1 && m.splits <= kGroupMaxSplits && m.tiles_per_split >= 1);
    CHECK(m.blocks == m.otiles * m.ctiles * m.splits && m.fin_blocks >= 1);
    CHECK((long long)m.splits * m.tiles_per_split >= m.ntiles);
    CHECK((long long)(m.splits - 1) * m.tiles_per_split < m.ntiles);   // no empty split
    CHECK(m.ntiles == s[i].nuse * m.use_tiles && m.use_tiles == s[i].B * m.tiles_img);
    CHECK(m.otiles * 64 >= s[i].Cout && m.ctiles * 64 >= s[i].Cin);
    CHECK(m.finish_q == 1 || m.finish_q == 2 || m.finish_q == 4);
    blocks += m.blocks;
    fin += m.fin_blocks;
    nuse += s[i].nuse;
    cover[i].assign((size_t)m.otiles * m.ctiles * m.ntiles, 0);
    const size_t wbytes = (size_t)m.splits * s[i].Cout * s[i].Cin * T * sizeof(float);
    const size_t bbytes = (size_t)m.splits * s[i].Cout * sizeof(float);
    CHECK(m.part_off % 256 == 0 && m.bpart_off % 256 == 0);
    regions.push_back({m.part_off, m.part_off + wbytes});
    regions.push_back({m.bpart_off, m.bpart_off + bbytes});
  }
  CHECK(blocks == pl.blocks && fin == pl.fin_blocks && nuse == pl.nuse && nuse <= kGroupUses);
  // one wave: at most `target` blocks, unless the (o, c) tiles alone exceed it
  bool unsplit = true;
  for (int i = 0; i < n; ++i) unsplit = unsplit && pl.m[i].splits == 1;
  CHECK(pl.blocks <= target || unsplit);
  std::sort(regions.begin(), regions.end());
  for (size_t r = 0; r < regions.size(); ++r) {
    CHECK(regions[r].second <= pl.bytes);
    if (r) CHECK(regions[r - 1].second <= regions[r].first);
  }
  // the kernel's prologue, block by block
  for (int id = 0; id < pl.blocks; ++id) {
    int mi = 0;
    for (int i = 1; i < kGroupMembers; ++i) mi += id >= block0[i] ? 1 : 0;
    CHECK(mi < n);
    const WgGroupMemberPlan& m = pl.m[mi];
    const int local = id - m.block0, noc = m.otiles * m.ctiles;
    CHECK(local >= 0 && local < m.blocks);
    const int by = local / noc, t = local - by * noc;
    const int ot = t % m.otiles, ct = t / m.otiles;
    CHECK(by < m.splits && ot < m.otiles && ct < m.ctiles);
    // split `by` takes every splits-th pixel tile
    const int count = (m.ntiles - by + m.splits - 1) / m.splits;
    CHECK(count >= 1 && count <= m.tiles_per_split);
    for (int tl = 0; tl < count; ++tl) {
      const int tile = by + tl * m.splits;
      CHECK(tile < m.ntiles);
      const int u = tile / m.use_tiles;
      CHECK(u < s[mi].nuse && m.use0 + u < kGroupUses);
      ++cover[mi][((size_t)ot * m.ctiles + ct) * m.ntiles + tile];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int c : cover[i]) CHECK(c == 1);
  // the finish's block -> member mapping
  for (int id = 0; id < pl.fin_blocks; ++id) {
    int mi = 0;
    for (int i = 1; i < kGroupMembers; ++i) mi += id >= fin0[i] ? 1 : 0;
    CHECK(mi < n && id - pl.m[mi].fin0 >= 0 && id - pl.m[mi].fin0 < pl.m[mi].fin_blocks);
  }
}

int main() {
  typedef std::vector<WgGroupShape> G;   // {nuse, B, H, W, Cin, Cout}
  // the GPU tests' groups (tests/test_wgrad_group.py)
  check(G{{1, 3, 7, 13, 48, 45}, {1, 1, 16, 24, 64, 130}, {3, 2, 9, 9, 70, 64}}, 3, 3, 256);
  check(G{{1, 1, 8, 8, 16, 24}, {2, 2, 10, 12, 26, 32}}, 3, 3, 256);
  for (int k = 0; k < 3; ++k) {
    const int KH = k == 1 ? 5 : 1, KW = k == 0 ? 5 : 1;
    check(G{{1, 2, 5, 19, 33, 70}, {2, 1, 10, 7, 66, 20}}, KH, KW, 256);
    check(G{{1, 2, 5, 19, 130, 9}, {1, 1, 10, 7, 7, 65}}, KH, KW, 256);
  }
  check(G(kGroupMembers, WgGroupShape{1, 1, 5, 6, 3, 4}), 3, 3, 256);
  check(G{{1, 1, 5, 6, 3, 4}}, 3, 3, 256);
  // the groups of the benchmark step (KITTI self-supervised, 2 + 4 frames of
  // 192 x 640, 8 iterations; profiles/wgrad_group_bench.txt): the encoders'
  // single-use 3x3 convs ...
  const WgGroupShape f64 = {1, 6, 48, 160, 64, 64}, f128 = {1, 6, 24, 80, 128, 128}, f256 = {1, 6, 12, 40, 256, 256};
  const WgGroupShape c64 = {1, 4, 48, 160, 64, 64}, c128 = {1, 4, 24, 80, 128, 128}, c256 = {1, 4, 12, 40, 256, 256};
  const WgGroupShape d64 = {1, 2, 48, 160, 64, 64}, d128 = {1, 2, 24, 80, 128, 128}, d256 = {1, 2, 12, 40, 256, 256};
  check(G{f64, f64, f64, f64}, 3, 3, 256);
  check(G{{1, 4, 24, 80, 128, 6}, f128, f256, f256, f256, f128, f128, f128}, 3, 3, 256);
  check(G{{8, 4, 24, 80, 64, 6}, {1, 4, 24, 80, 128, 96}, c256, c256, c256, c128, c128, c128}, 3, 3, 256);
  check(G{c64, c64, c64, c64, {1, 2, 24, 80, 128, 96}, d256, d256, d256}, 3, 3, 256);
  check(G{d128, d128, d128, d64, d64, d64, d64}, 3, 3, 256);
  // ... and the update blocks' weights, 8 uses each: heads and projection
  // encoders (relu), SepConvGRU gates and candidates, the mask and output convs
  check(G{{8, 2, 24, 80, 64, 192}, {8, 2, 24, 80, 128, 63}, {8, 2, 24, 80, 64, 64}}, 3, 3, 256);
  check(G{{8, 4, 24, 80, 64, 64}, {8, 4, 24, 80, 128, 58}, {8, 4, 24, 80, 64, 64}}, 3, 3, 256);
  check(G{{8, 2, 24, 80, 64, 64}, {1, 2, 24, 80, 128, 256}, {1, 2, 24, 80, 128, 128}, {1, 4, 24, 80, 256, 128},
          {1, 6, 24, 80, 256, 128}, {1, 6, 24, 80, 256, 128}}, 3, 3, 256);
  for (int B = 2; B <= 4; B += 2) {
    check(G{{8, B, 24, 80, 160, 128}, {8, B, 24, 80, 160, 64}}, 1, 5, 256);
    check(G{{8, B, 24, 80, 160, 128}, {8, B, 24, 80, 160, 64}}, 5, 1, 256);
    check(G{{8, B, 24, 80, 128, 64}}, 1, 1, 256);
  }
  check(G{{8, 2, 24, 80, 128, 576}, {1, 2, 24, 80, 256, 576}}, 1, 1, 256);
  check(G{{8, 2, 24, 80, 64, 1}}, 3, 3, 256);
  // sweep: member counts, ragged sizes, channel counts around the 64 tile, targets
  unsigned long long rng = 12345;
  auto next = [&](int lo, int hi) {
    rng = rng * 6364136223846793005ULL + 1442695040888963407ULL;
    return lo + (int)((rng >> 33) % (unsigned)(hi - lo + 1));
  };
  const int kshape[4][2] = {{1, 1}, {1, 5}, {5, 1}, {3, 3}};
  const int targets[4] = {1, 64, 256, 1024};
  for (int it = 0; it < 600; ++it) {
    const int n = next(1, kGroupMembers);
    G g;
    int slots = kGroupUses;
    for (int i = 0; i < n; ++i) {
      const int room = std::min(kGroupUsesPerMember, slots - (n - 1 - i));
      const int nuse = next(1, it % 3 ? std::min(room, 3) : room);
      slots -= nuse;
      static const int chans[] = {1, 3, 63, 64, 65, 128, 130, 257};
      g.push_back({nuse, next(1, 4), next(1, 40), next(1, 70), chans[next(0, 7)], chans[next(0, 7)]});
    }
    check(g, kshape[it & 3][0], kshape[it & 3][1], targets[(it >> 2) & 3]);
  }
  // what the planner must refuse
  WgGroupPlan pl;
  const WgGroupShape one = {1, 1, 8, 8, 8, 4}, many = {16, 1, 8, 8, 8, 4};
  const WgGroupShape nine[kGroupMembers + 1] = {one, one, one, one, one, one, one, one, one};
  const WgGroupShape over[2] = {many, many};
  WgGroupShape zero = one, seventeen = one;
  zero.nuse = 0;
  seventeen.nuse = 17;
  CHECK(!wgrad_group_plan(nullptr, 1, 3, 3, 256, &pl) && !wgrad_group_plan(&one, 0, 3, 3, 256, &pl));
  CHECK(!wgrad_group_plan(nine, kGroupMembers + 1, 3, 3, 256, &pl) && !wgrad_group_plan(&one, 1, 7, 7, 256, &pl));
  CHECK(!wgrad_group_plan(over, 2, 3, 3, 256, &pl));
  CHECK(!wgrad_group_plan(&zero, 1, 3, 3, 256, &pl) && !wgrad_group_plan(&seventeen, 1, 3, 3, 256, &pl));
  printf("wgrad_group_plan_check: %lld plans ok (%d members, %d use slots)\n", g_plans, kGroupMembers, kGroupUses);
  return 0;
}
