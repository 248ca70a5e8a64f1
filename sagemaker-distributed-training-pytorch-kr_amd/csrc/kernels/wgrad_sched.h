// Work-item scheduling shared by the weight-gradient GEMM kernels (wgrad_gemm.hip: 16-bit operands,
// wgrad_fp8.hip: FP8 operands): the counted vmcnt wait of the LDS-DMA stage ring, the XCD-aware
// block remap, the (n-group, k, n-in-group) tile order and the tail-split switch.
#pragma once
#include <cstdlib>

#include "common.h"

namespace smdt {
namespace wg {

using lds_void = __attribute__((address_space(3))) void;

// s_waitcnt with vmcnt = n and the other counters left alone (gfx9 encoding).
template <int n>
__device__ __forceinline__ void wait_vm() {
  static_assert(n >= 0 && n < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((n & 15) | ((n >> 4) << 14) | (7 << 4) | (15 << 8));
}

// XCD-aware bijective remap: hardware dispatches block b to XCD b % 8; give each XCD a
// contiguous range of work items.
__device__ __forceinline__ int xcd_remap(int orig, int nblocks) {
  const int xcd = orig & 7, q = nblocks >> 3, rem = nblocks & 7;
  return (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
}

// Tile t of an ntn x ntk grid in groups of gn n-tiles x all k-tiles, n fastest inside a group.
__device__ __forceinline__ void tile_coords(int t, int ntn, int ntk, int gn, int& tn, int& tk) {
  const int grp = t / (gn * ntk);
  const int gn_eff = min(gn, ntn - grp * gn);
  const int tg = t - grp * gn * ntk;
  tn = grp * gn + tg % gn_eff;
  tk = tg / gn_eff;
}

inline int group_width(int ntk) { return ntk <= 4 ? 8 : 4; }

// SMDT_WGRAD_TAIL_SPLIT=0 turns the split of a grouped launch's tail tiles off.
inline bool tail_split_enabled() {
  static const int on = [] {
    const char* v = getenv("SMDT_WGRAD_TAIL_SPLIT");
    return (v && v[0] == '0') ? 0 : 1;
  }();
  return on != 0;
}

// Tail split of a grouped launch of `tiles` output tiles on R CUs: the r = tiles mod R tail tiles
// are cut along m into `splits` pieces of `mps` stages (at least 8 stages each, at most 16
// pieces); splits = 1 leaves every tile whole.
inline void tail_split(int tiles, int R, int max_stages, int& splits, int& mps) {
  const int r = tiles % R;
  splits = 1;
  mps = 0;
  if (r > 0 && tail_split_enabled()) {
    splits = R / r;
    if (splits > 16) splits = 16;
    if (splits > max_stages / 8) splits = max_stages / 8;
    if (splits > 1) {
      mps = (max_stages + splits - 1) / splits;
      splits = (max_stages + mps - 1) / mps;
    }
  }
  if (splits < 1) splits = 1;
}

}  // namespace wg
}  // namespace smdt
