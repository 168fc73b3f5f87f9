// Tile schedule of the x3 GEMMs (gemm_x3.hip): which logical workgroup runs which tiles, in which
// order. Host-callable, so nos_gemm_x3_schedule reports the launch's own schedule through the very
// functions the kernels run (tests/test_gemm_x3_schedule.py walks it exhaustively on the CPU), as
// streamk.h does for the stream-K split.
#pragma once
#include "pin.h"

// Logical tile order: xcd_major_n (pin.h) deals workgroups round-robin over the XCDs (phys % nx =
// XCD, observed placement — speed only, never correctness), so XCD x gets a contiguous logical range:
// a band of whole tile rows whose A rows stay in that XCD's L2 while it sweeps the weight columns.

// Persistent grids: workgroup w's tiles are base + i*stride, i < count — the XCD's band again, dealt
// over the XCD's P/nx workgroups (nx XCDs: 8, or the pinned partition's; P % nx == 0, otherwise a
// plain w + i*P sweep).
__host__ __device__ __forceinline__ void xcd_band(int w, int P, int nx, int tiles, int& base, int& stride, int& count) {
  if (P % nx) {
    base = w, stride = P, count = w < tiles ? (tiles - w + P - 1) / P : 0;
    return;
  }
  const int x = w % nx, li = w / nx, px = P / nx, q = tiles / nx, r = tiles % nx;
  const int n = q + (x < r ? 1 : 0);
  base = x * q + min(x, r) + li, stride = px, count = li < n ? (n - li + px - 1) / px : 0;
}

// Grouped tile order: logical tile t walks GROUP tile rows down a column before moving right, so
// the tiles an XCD runs at once cover GROUP rows x (its workgroups / GROUP) columns — A and W
// slices that fit its 4 MB L2 together — instead of one row of tiles sweeping all of W. GROUP
// rides in bits 8-15 of the epilogue word (1 = plain row-major order).
__host__ __device__ __forceinline__ void tile_rc(int t, int tiles_m, int tiles_n, int group, int& mt, int& nt) {
  if (group <= 1) {
    mt = t / tiles_n, nt = t % tiles_n;
    return;
  }
  const int per = group * tiles_n, g = t / per, r0 = g * group, gs = min(tiles_m - r0, group), o = t - g * per;
  mt = r0 + o % gs, nt = o / gs;
}

// The one unit of logical workgroup `id` of `n` in a one-tile-per-workgroup launch of `tiles` tiles:
// unit = (logical tile t, split sp), a tile's splits adjacent (one XCD's L2); tile_rc places t.
// False: no unit (the launch is rounded up to whole rounds of XCDs).
__host__ __device__ __forceinline__ bool x3_unit(int id, int n, int nx, int tiles, int splits, int& t, int& sp) {
  const int u = xcd_major_n(id, n, nx);
  if (u >= tiles * splits) return false;
  t = u / splits, sp = u - t * splits;
  return true;
}

// workgroups of a persistent launch asked for `grid`: never more than tiles, never none
inline int x3s_grid(int grid, int tiles) {
  const int g = grid < tiles ? grid : tiles;
  return g > 1 ? g : 1;
}
