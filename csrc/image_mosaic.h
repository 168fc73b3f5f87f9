// The mosaic of the image library (image.hip): the detections of selected labels pixelated in the frame's own planes.
//  * mosaic_k<Surface> — one workgroup of 256 threads per 64 x 64 tile of luma pixels on the frame's lattice, so the
//    grid depends on the frame's size alone. The rule is exact integers; ops/image.py's mosaic states it in full.
//
// Why painting in place is race-free. Every allowed cell (4, 8, 16, 32, 64) divides the tile, the lattice of cells and
// the lattice of tiles both start at pixel (0, 0), a chroma cell lies exactly under its luma cell (cell >> hsub >= 2) and
// a 4:2:2 macropixel never straddles a multiple of 64. So every sample a workgroup reads or writes belongs to a pixel of
// its own tile: no two workgroups touch the same byte, and inside a workgroup every read of the frame lies before the
// barrier that ends staging and every write behind the barrier that ends the reduction. No atomics, no traffic between
// workgroups, no second buffer.
//
// A workgroup's steps:
//  1. Row list. The rows the rule selects (select_rect: overlay's filters with select[label] in place of the mode)
//     whose rectangle, clipped to the frame, touches the tile are kept in LDS, by the ballot compaction per 256 rows that
//     overlay_k uses (copied here, so that overlay_k is untouched). Only the rectangle is kept, clipped to the tile: four
//     coordinates of 0..63 in one word. A tile that lists nothing returns before it has read a byte of the frame.
//  2. Cell mask. One byte per cell of the tile (256 at cell 4). 256 / cells threads share a cell and stride through the
//     list; a hit stores 1 (several threads may store the same 1). A listed rectangle holds a pixel of the tile, so a
//     tile with a list has a marked cell.
//  3. Stage. The tile's in-frame samples go to LDS as 16-bit codes, luma 64 x 64 and chroma at its own resolution, one
//     array per colour component. Each plane is walked row by row in dwords (stage_rows): one aligned 32-bit load where
//     the row's first byte and the pitch are multiples of four and the dword lies inside the tile's row, else byte loads
//     of the bytes inside it. The structs of image_overlay.h give the addresses (PackedDst / YuvDst: the same planes,
//     pitches, orders and shift their store uses). A per-sample load() beside store() would be one byte load per sample
//     and three walks over packed pixels; the row walk reads every byte of the tile once. The alpha byte of a four-byte
//     pixel travels with its dword and is dropped: it reaches no result and is never written.
//  4. Reduce, separably, in int32 (the largest sum is 64 * 64 * 4095 < 2^24). Pass one: a thread per (row, cell column,
//     component) sums the cell's codes of its row, only where the cell is marked. Pass two: a thread per (cell,
//     component) sums the rows' partials and divides once, unsigned: m = (sum + n / 2) / n, n the cell's samples inside
//     the frame. Matrix instructions do not fit: the sums must be exact and are tiny beside the traffic.
//  5. Write. Behind a barrier each thread stores, for its 16 pixels, those in marked cells through PackedDst / YuvDst's
//     own store, which has the guards the rule needs (a chroma sample is stored by its owner pixel's thread only);
//     y < h && x < w is tested here.
//
// LDS banks. A row of codes is MROW = 66 halfwords = 33 banks (odd), and in pass one a wave's lanes are consecutive
// rows: their reads hit banks 33 row + c, all different for up to 64 rows on 64 banks and for each half-wave on 32. Where
// a chroma plane has 32 rows a wave is rows 0..31 of U and of V; the component arrays are MPLANE = 64 * 66 + 64
// halfwords apart (32 banks mod 64), and so are the partials' (MPARTC), which pass one writes to consecutive words.
// Pass two's lanes run down a cell column first, then across (a column is MPART = 65 words). Checked by enumerating on
// the host, for every cell size and subsampling, the bank of every lane of every wave in both passes. Pass one, reads and
// writes: no two lanes of a wave share a bank on a 64-bank model, none of a half-wave on a 32-bank model. Pass two is
// not free, and was left so because it is tiny (768 threads of 4 reads at cell 4, 3 threads of 64 at cell 64, beside
// 12288 codes staged): on 64 banks it is free at cells 4 and 8 but for 4:2:0 (two lanes per bank) and has up to three
// lanes per bank from cell 16 up; on 32 banks two at cells 4 and 8 and up to six at cell 32, where it is 12 threads.
//
// LDS size. Codes 25.7 KB, partials 12.7 KB, means and marks 1.8 KB: 40.2 KB, four workgroups a CU, which also bounds
// the tiles that return right after the row scan. The row list lives in the partials' words for that reason: with 4 KB
// of its own (44.3 KB, three workgroups a CU) the 400-row 2160p NV12 scene took 35.2 us on the whole GPU and 195.7 on 32
// CUs, against 30.8 and 156.1 as it stands (tools/kbench.py --rows mosaic, medians of three rounds).
// Included by image.hip alone, after image_overlay.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "image_overlay.h"

namespace {
// threads of a workgroup; the side of its tile; halfwords of a row and of a component's array of codes; words of a
// column of partials and of a component's partials (16 columns)
constexpr int MT = 256, MTILE = 64, MROW = 66, MPLANE = MTILE * MROW + 64, MPART = 65, MPARTC = 16 * 66;
constexpr int MOSAIC_MIN_CELL = 4;
static_assert(MT == 4 * MTILE && MTILE % 64 == 0, "a wave writes one row of the tile, four rows a pass");
static_assert((MROW / 2) % 2 == 1 && (MPLANE / 2) % 64 == 32 && MPARTC % 64 == 32 && MPARTC >= 16 * MPART, "banks");

// The lists as OverlayArgs holds them; select [L] uint8 (non-zero: pixelate the label); cell: 4, 8, 16, 32 or 64;
// mask: 2^depth - 1 of a 16-bit surface's samples.
struct MosaicArgs {
  const int* count;
  const float* scores;
  const int* labels;
  const float* boxes;
  const int* track_id;
  const int* track_hits;
  const uint8_t* select;
  int N, L, min_hits, h, w, cell, mask;
};

// Row r's rectangle (inclusive, not clipped); false when the rule does not select the row. The filters and the
// rectangle are make_record's.
__device__ __forceinline__ bool select_rect(const MosaicArgs& a, int r, int& x0, int& y0, int& x1, int& y1) {
  if (!(a.scores[r] > 0.f)) return false;  // a NaN is not selected
  const int label = a.labels[r];
  if (label < 0 || label >= a.L || a.select[label] == 0) return false;
  if (a.track_id != nullptr && (a.track_id[r] <= 0 || a.track_hits[r] < a.min_hits)) return false;
  float c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c[i] = a.boxes[4 * size_t(r) + i];
    if (!isfinite(c[i])) return false;
    c[i] = fminf(fmaxf(c[i], -OVERLAY_CLAMP), OVERLAY_CLAMP);
  }
  x0 = int(floorf(c[0])), y0 = int(floorf(c[1]));
  x1 = int(ceilf(c[2])) - 1, y1 = int(ceilf(c[3])) - 1;
  return x1 >= x0 && y1 >= y0;
}

// rows x bytes from p, rows pitch apart, four bytes a thread: put(row, b, v, n) gets bytes b .. b + n - 1 of a row in
// the low n bytes of v. No byte outside the rows' bytes is read.
template <class F>
__device__ __forceinline__ void stage_rows(const uint8_t* p, long long pitch, int rows, int bytes, F put) {
  const bool wide = ((reinterpret_cast<uintptr_t>(p) | uintptr_t(pitch)) & 3) == 0;
  const int per = (bytes + 3) >> 2;
  for (int i = threadIdx.x; i < rows * per; i += MT) {
    const int row = i / per, b = 4 * (i - row * per), n = min(4, bytes - b);
    const uint8_t* q = p + row * pitch + b;
    uint32_t v = 0;
    if (wide && n == 4) {
      v = *reinterpret_cast<const uint32_t*>(q);
    } else {
      for (int k = 0; k < n; ++k) v |= uint32_t(q[k]) << (8 * k);
    }
    put(row, b, v, n);
  }
}

// The samples of sb bytes in the n bytes of v that start at byte b of a row: put(sample index in the row, code).
template <class F>
__device__ __forceinline__ void each_sample(int sb, int shift, int mask, int b, uint32_t v, int n, F put) {
  if (sb == 2) {
    for (int k = 0; k < n; k += 2) put((b + k) >> 1, int(((v >> (8 * k)) & 0xffffu) >> shift) & mask);
  } else {
    for (int k = 0; k < n; ++k) put(b + k, int((v >> (8 * k)) & 255u));
  }
}

__device__ __forceinline__ void mosaic_sub(const PackedDst&, int& hs, int& vs) { hs = 0, vs = 0; }
__device__ __forceinline__ void mosaic_sub(const YuvDst& d, int& hs, int& vs) { hs = d.hsub, vs = d.vsub; }

// The th x tw in-frame pixels of the tile at (ty0, tx0) as codes: component c's sample (row, col) of the tile at
// code[c * MPLANE + row * MROW + col].
__device__ __forceinline__ void mosaic_stage(const PackedDst& d, const MosaicArgs&, int ty0, int tx0, int th, int tw,
                                             uint16_t* code) {
  const int C = d.C, r = d.r;
  stage_rows(d.s.p + ty0 * d.s.pitch + (long long)tx0 * C, d.s.pitch, th, tw * C, [=](int row, int b, uint32_t v, int n) {
    for (int k = 0; k < n; ++k) {
      const int at = b + k, px = C == 4 ? at >> 2 : at / 3, ch = at - px * C;
      const int comp = ch == r ? 0 : ch == 1 ? 1 : ch == 2 - r ? 2 : -1;
      if (comp >= 0) code[comp * MPLANE + row * MROW + px] = uint16_t((v >> (8 * k)) & 255u);
    }
  });
}

__device__ __forceinline__ void mosaic_stage(const YuvDst& d, const MosaicArgs& a, int ty0, int tx0, int th, int tw,
                                             uint16_t* code) {
  const int sb = d.sb, shift = d.shift, mask = a.mask, order = d.order;
  if (d.layout == 2) {
    // a macropixel of four bytes, as YuvDst::store lays it out; its second luma may lie behind the frame's last column
    const int yo = order == 1 ? 1 : 0, uo = order == 0 ? 1 : order == 1 ? 0 : 3, vo = order == 0 ? 3 : order == 1 ? 2 : 1;
    stage_rows(d.pl[0].p + ty0 * d.pl[0].pitch + 2LL * tx0, d.pl[0].pitch, th, 4 * ((tw + 1) >> 1),
               [=](int row, int b, uint32_t v, int n) {
                 for (int k = 0; k < n; ++k) {
                   const int at = b + k, mp = at >> 2, pos = at & 3;
                   const uint16_t c = uint16_t((v >> (8 * k)) & 255u);
                   if (pos == uo) code[MPLANE + row * MROW + mp] = c;
                   else if (pos == vo) code[2 * MPLANE + row * MROW + mp] = c;
                   else code[row * MROW + 2 * mp + ((pos - yo) >> 1)] = c;
                 }
               });
    return;
  }
  stage_rows(d.pl[0].p + ty0 * d.pl[0].pitch + (long long)tx0 * sb, d.pl[0].pitch, th, tw * sb,
             [=](int row, int b, uint32_t v, int n) {
               each_sample(sb, shift, mask, b, v, n, [=](int e, int c) { code[row * MROW + e] = uint16_t(c); });
             });
  const int cy0 = ty0 >> d.vsub, cx0 = tx0 >> d.hsub;
  const int tch = (th + (1 << d.vsub) - 1) >> d.vsub, tcw = (tw + (1 << d.hsub) - 1) >> d.hsub;
  if (d.layout == 1) {
    // pairs: U at sample 2 cx + order
    stage_rows(d.pl[1].p + cy0 * d.pl[1].pitch + 2LL * cx0 * sb, d.pl[1].pitch, tch, 2 * tcw * sb,
               [=](int row, int b, uint32_t v, int n) {
                 each_sample(sb, shift, mask, b, v, n, [=](int e, int c) {
                   code[((e & 1) == order ? 1 : 2) * MPLANE + row * MROW + (e >> 1)] = uint16_t(c);
                 });
               });
    return;
  }
  for (int i = 1; i < 3; ++i)
    stage_rows(d.pl[i].p + cy0 * d.pl[i].pitch + (long long)cx0 * sb, d.pl[i].pitch, tch, tcw * sb,
               [=](int row, int b, uint32_t v, int n) {
                 each_sample(sb, shift, mask, b, v, n,
                             [=](int e, int c) { code[i * MPLANE + row * MROW + e] = uint16_t(c); });
               });
}

// The trip count of the loop that holds barriers (n, the rows) is read from LDS by all threads, and so is what the
// loop adds to the list's length; every return is taken by the whole workgroup.
template <class Dst>
__global__ __launch_bounds__(MT) void mosaic_k(MosaicArgs a, Dst dst) {
  __shared__ uint16_t s_code[3 * MPLANE];
  __shared__ int s_part[3 * MPARTC];
  // the list lives in the partials' words: its last read (the cell mask) and pass one's first write lie on either
  // side of the barrier that ends staging
  static_assert(3 * MPARTC >= OMAX, "the list fits the partials");
  uint32_t* const s_rect = reinterpret_cast<uint32_t*>(s_part);
  __shared__ uint16_t s_mean[3 * 256];
  __shared__ uint8_t s_mark[256];
  __shared__ int s_wave[MT / 64], s_n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (a.w + MTILE - 1) / MTILE;
  const int ty0 = int(blockIdx.x) / tiles_x * MTILE, tx0 = int(blockIdx.x) % tiles_x * MTILE;
  const int th = min(MTILE, a.h - ty0), tw = min(MTILE, a.w - tx0);  // the tile's pixels inside the frame
  if (tid == 0) s_n = min(max(a.count[0], 0), a.N);
  s_mark[tid] = 0;
  __syncthreads();
  const int n = s_n;
  int m = 0;  // rows listed so far: the same in every thread
  for (int base = 0; base < n; base += MT) {
    const int r = base + tid;
    int x0, y0, x1, y1;
    bool keep = r < n && select_rect(a, r, x0, y0, x1, y1);
    if (keep) {
      x0 = max(x0 - tx0, 0), y0 = max(y0 - ty0, 0), x1 = min(x1 - tx0, tw - 1), y1 = min(y1 - ty0, th - 1);
      keep = x0 <= x1 && y0 <= y1;
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    int off = m;
    for (int k = 0; k < MT / 64; ++k) {
      if (k < wave) off += s_wave[k];
      m += s_wave[k];
    }
    if (keep) s_rect[off + __popcll(mask & ((1ull << lane) - 1ull))] = uint32_t(x0 | x1 << 8 | y0 << 16 | y1 << 24);
    __syncthreads();  // the list is written, and s_wave is free for the next 256 rows
  }
  if (m == 0) return;

  // the cell mask: lg = log2(cell); the tile has ncc x ncc cells, cell (ci, cc) at s_mark[ci * ncc + cc]
  const int lg = __ffs(a.cell) - 1, lgc = 6 - lg, ncc = 1 << lgc, ncell = ncc * ncc;
  {
    const int share = MT >> (2 * lgc), k = tid / share;
    const int cx = (k & (ncc - 1)) << lg, cy = (k >> lgc) << lg;
    bool hit = false;
    for (int i = tid % share; i < m && !hit; i += share) {
      const uint32_t q = s_rect[i];
      hit = int(q & 255) < cx + a.cell && int((q >> 8) & 255) >= cx && int((q >> 16) & 255) < cy + a.cell &&
            int(q >> 24) >= cy;
    }
    if (hit) s_mark[k] = 1;
  }
  mosaic_stage(dst, a, ty0, tx0, th, tw, s_code);
  __syncthreads();  // the last read of the frame lies before this barrier

  int hs, vs;
  mosaic_sub(dst, hs, vs);
  // pass one: luma (g = 0), then both chroma components (g = 1); a wave's lanes are consecutive rows
  for (int g = 0; g < 2; ++g) {
    const int ghs = g ? hs : 0, gvs = g ? vs : 0;
    const int lgr = 6 - gvs, rows = (th + (1 << gvs) - 1) >> gvs, cols = (tw + (1 << ghs) - 1) >> ghs;
    const int cwid = a.cell >> ghs;
    for (int i = tid; i < ((1 + g) * ncc) << lgr; i += MT) {
      const int row = i & ((1 << lgr) - 1), j = i >> lgr, comp = g + (j & g), cc = j >> g;
      int sum = 0;
      if (row < rows && s_mark[(row >> (lg - gvs)) * ncc + cc]) {
        const uint16_t* q = s_code + comp * MPLANE + row * MROW + cc * cwid;
        const int lim = min(cwid, cols - cc * cwid);
        for (int x = 0; x < lim; ++x) sum += q[x];
      }
      s_part[comp * MPARTC + cc * MPART + row] = sum;
    }
  }
  __syncthreads();
  // pass two: a thread per marked (cell, component), down a cell column first
  for (int i = tid; i < 3 * ncell; i += MT) {
    const int comp = i >> (2 * lgc), ci = i & (ncc - 1), cc = (i >> lgc) & (ncc - 1);
    if (!s_mark[ci * ncc + cc]) continue;
    const int ghs = comp ? hs : 0, gvs = comp ? vs : 0;
    const int rows = (th + (1 << gvs) - 1) >> gvs, cols = (tw + (1 << ghs) - 1) >> ghs;
    const int cv = a.cell >> gvs, cwid = a.cell >> ghs;
    const int nr = min(cv, rows - ci * cv), nc = min(cwid, cols - cc * cwid);
    int sum = 0;
    for (int j = 0; j < nr; ++j) sum += s_part[comp * MPARTC + cc * MPART + ci * cv + j];
    const unsigned cnt = unsigned(nr * nc);  // a marked cell holds a pixel of the frame, so its first: cnt >= 1
    s_mean[comp * 256 + ci * ncc + cc] = uint16_t((unsigned(sum) + cnt / 2) / cnt);
  }
  __syncthreads();
  for (int pass = 0; pass < MTILE / 4; ++pass) {
    const int ly = pass * 4 + wave, lx = lane;
    if (ly >= th || lx >= tw) continue;
    const int k = (ly >> lg) * ncc + (lx >> lg);
    if (!s_mark[k]) continue;
    const int col[3] = {s_mean[k], s_mean[256 + k], s_mean[512 + k]};
    dst.store(ty0 + ly, tx0 + lx, col);
  }
}
}  // namespace
