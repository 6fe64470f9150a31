// Launch plan of the grouped weight gradient (conv.hip: wgrad2_group_kernel):
// several weights of one kernel shape share ONE wave of blocks and one finish.
// Plain host C++ (no device code): tools/wgrad_group_plan_check.cpp sweeps it
// on the CPU.
#pragma once
#include <cstddef>

namespace dro {

constexpr int kGroupMembers = 8;    // weights per grouped launch
constexpr int kGroupUses = 24;      // use slots per grouped launch, over all members
constexpr int kGroupUsesPerMember = 16;
constexpr int kGroupTarget = 256;   // blocks per launch: one 8-wave block per CU
constexpr int kGroupMaxSplits = 256;

struct WgGroupShape {   // one member: a weight [Cout][Cin][KH][KW] with nuse uses of B x H x W pixels
  int nuse, B, H, W, Cin, Cout;
};

struct WgGroupMemberPlan {
  int tiles_x, tiles_img;   // TH x TW pixel tiles per row / per image
  int use_tiles, ntiles;    // pixel tiles per use, over all uses
  int otiles, ctiles;       // 64-channel tiles of Cout / Cin
  int tiles_per_split, splits;   // split s takes pixel tiles s, s + splits, ...: at most tiles_per_split
  int block0, blocks;       // blocks [block0, block0 + otiles * ctiles * splits) of the grid
  int finish_q;             // lanes per element of the split sum (1, 2, 4)
  int fin0, fin_blocks;     // blocks of the finish launch
  int use0;                 // first use slot
  size_t part_off, bpart_off;   // byte offsets into the workspace: [splits][T][Cout][Cin], [splits][Cout]
};

struct WgGroupPlan {
  int nmember, blocks, fin_blocks, nuse;
  size_t bytes;             // workspace
  WgGroupMemberPlan m[kGroupMembers];
};

inline bool wgrad_group_shape_ok(int KH, int KW) {
  return (KH == 1 && KW == 5) || (KH == 5 && KW == 1) || (KH == 3 && KW == 3) || (KH == 1 && KW == 1);
}

inline size_t wgrad_group_align(size_t n) { return (n + 255) & ~(size_t)255; }

// Every block is a 64 x 64 x T channel tile over a run of pixel tiles, so a
// block's cost is its pixel tiles: the wave of `target` blocks is shared out
// with one run length for all members (tps), and each member then balances
// its own runs.  false: not a grouped shape, or the members / use slots do
// not fit one launch (the caller cuts the group).
inline bool wgrad_group_plan(const WgGroupShape* s, int n, int KH, int KW, int target, WgGroupPlan* pl) {
  if (!s || !pl || n < 1 || n > kGroupMembers || !wgrad_group_shape_ok(KH, KW) || target < 1) return false;
  const int TH = (KW == 1 || (KH == 3 && KW == 3)) ? 8 : 4, TW = 64 / TH, T = KH * KW;
  long long work = 0;
  int nuse = 0;
  for (int i = 0; i < n; ++i) {
    if (s[i].nuse < 1 || s[i].nuse > kGroupUsesPerMember || s[i].B < 1 || s[i].H < 1 || s[i].W < 1 ||
        s[i].Cin < 1 || s[i].Cout < 1)
      return false;
    WgGroupMemberPlan& m = pl->m[i];
    m.tiles_x = (s[i].W + TW - 1) / TW;
    m.tiles_img = ((s[i].H + TH - 1) / TH) * m.tiles_x;
    m.use_tiles = s[i].B * m.tiles_img;
    m.ntiles = s[i].nuse * m.use_tiles;
    m.otiles = (s[i].Cout + 63) / 64;
    m.ctiles = (s[i].Cin + 63) / 64;
    m.use0 = nuse;
    nuse += s[i].nuse;
    work += (long long)m.ntiles * m.otiles * m.ctiles;
  }
  if (nuse > kGroupUses) return false;
  // The smallest run length whose blocks fit the wave: the kernel runs one
  // block per CU, so a block past `target` waits for a free CU and the launch
  // takes two runs instead of one (rounding every member's split count up can
  // add a block per (o, c) tile).  With more (o, c) tiles than `target` every
  // member gets one split.
  long long tps = (work + target - 1) / target, max_tiles = 1;
  for (int i = 0; i < n; ++i) max_tiles = pl->m[i].ntiles > max_tiles ? pl->m[i].ntiles : max_tiles;
  auto blocks_at = [&](long long t) {
    long long b = 0;
    for (int i = 0; i < n; ++i) {
      long long sp = (pl->m[i].ntiles + t - 1) / t;
      b += (long long)pl->m[i].otiles * pl->m[i].ctiles * (sp > kGroupMaxSplits ? kGroupMaxSplits : sp);
    }
    return b;
  };
  if (blocks_at(max_tiles) > target) tps = max_tiles;
  while (tps < max_tiles && blocks_at(tps) > target) ++tps;
  int block = 0, fin = 0;
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    WgGroupMemberPlan& m = pl->m[i];
    long long sp = (m.ntiles + tps - 1) / tps;
    if (sp > kGroupMaxSplits) sp = kGroupMaxSplits;
    m.tiles_per_split = (int)((m.ntiles + sp - 1) / sp);
    m.splits = (m.ntiles + m.tiles_per_split - 1) / m.tiles_per_split;
    m.block0 = block;
    m.blocks = m.otiles * m.ctiles * m.splits;
    block += m.blocks;
    m.finish_q = m.splits >= 32 ? 4 : m.splits >= 8 ? 2 : 1;
    const long long total = (long long)s[i].Cout * s[i].Cin * T;
    long long fb = (total * m.finish_q + 255) / 256;
    if (fb > 4096) fb = 4096;
    m.fin0 = fin;
    m.fin_blocks = (int)fb;
    fin += m.fin_blocks;
    m.part_off = off;
    off += wgrad_group_align((size_t)m.splits * (size_t)total * sizeof(float));
    m.bpart_off = off;
    off += wgrad_group_align((size_t)m.splits * s[i].Cout * sizeof(float));
  }
  pl->nmember = n;
  pl->blocks = block;
  pl->fin_blocks = fin;
  pl->nuse = nuse;
  pl->bytes = off;
  return true;
}

}  // namespace dro
