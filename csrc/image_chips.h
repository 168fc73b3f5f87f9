// The chips of the image library (image.hip): the detections of selected labels cut out of the frame, each resampled
// to one fixed size, as RGB bytes. The first image kernel that writes a new tensor instead of the frame.
//  * chips_k<Src, source arguments, Yuv<...>> — one workgroup of 256 threads per (band of output rows, slot), so the
//    grid depends on the capacity and the chip size alone and a captured graph replays it. The rule is exact integers;
//    ops/image.py's chips states it in full.
//
// A workgroup's steps:
//  1. Slot. The rows the rule selects (select_rect of image_mosaic.h, then the margin and the clip to the frame:
//     chip_rect) are counted by the ballot compaction per 256 rows that overlay_k and mosaic_k use; the row whose rank
//     is the workgroup's slot leaves its rectangle in LDS. The scan stops behind that row, but in workgroup (0, 0),
//     which counts all rows and writes chip_count. Band 0 of a slot writes rows[slot] and rects[slot]. A slot without a
//     row stores zeros to its band of the chip and returns before it has read a byte of the frame.
//  2. Stream. The band's output rows j0 .. j1 - 1 cover source rows T0 .. T1 - 1 of the rectangle. They are taken in
//     chunks of CHIP_ROWS rows and, where the rectangle is wider than that, in chunks of CHIP_GROUPS column groups (256
//     columns). A column group is four columns of the *frame* (group g is columns 4 g .. 4 g + 3), whatever X0 is, so a
//     chroma pair lies under its luma; thread (row, group) stages it with the functions of image_stage.h (stage_yuv,
//     stage_yuv_bilinear, through hdr_pixel for PQ / HLG) or stage_packed here, 12 RGB bytes into LDS. Columns left of
//     X0 and right of X1 in the first and last group get bytes no later pass reads.
//  3. Horizontal pass. Thread (staged row, output column v, channel c) sums the source columns its output column
//     overlaps, restricted to the column chunk: whole columns weigh sw, the two ends the overlap's length, all from
//     v, bw, sw in integers (no taps from the host). The sums go to LDS as uint32 [row][v][c] and are added to across
//     column chunks by the thread that wrote them.
//  4. Vertical pass. A thread holds up to CHIP_NACC accumulators, outputs e = tid + 256 i of the band in the order
//     (output row, v, c), in registers across all chunks: for every source row of the chunk whose overlap with its
//     output row is positive it adds overlap x the row's horizontal sum. Shrinking, a source row feeds one or two
//     output rows; enlarging, an output row reads one or two source rows; the code is the same.
//  5. Store. One unsigned division per output: (sum + A / 2) / A with A = bh bw. sum <= 255 A and A <= 2^24 (the entry
//     refuses a larger frame), so everything fits uint32. Output e of the band is byte e of the band: consecutive lanes
//     store consecutive bytes.
//
// LDS: CHIP_ROWS x (CHIP_ROWW dwords staged + 3 sw dwords of sums), dynamic: 6.0 KB + 96 sw bytes — 12.2 KB at sw = 64,
// 30.6 KB at sw = 256. With the 160 KB of a CU that is 13 and 5 workgroups by LDS. Registers: 12 accumulators, 24 of
// their coordinates, 9 of the horizontal pass's columns, and what staging takes: the compiler reports 90 (packed) to 114
// (bilinear chroma) VGPRs by instantiation, nothing spilled to scratch, 4 to 5 waves a SIMD — 4 to 5 workgroups a CU,
// which binds before the LDS does at every chip width.
//
// LDS banks. Staging: lanes are consecutive groups of one row, 3 dwords apart, and 3 is coprime to the bank count:
// every one of store_rgb4's three stores is conflict-free; a staged row is CHIP_ROWW = 193 dwords (odd), so where a wave
// holds several rows (sw small) they start in different banks. Horizontal pass: lanes are consecutive (v, c); they read
// bytes 3 bw / sw apart per step of v. Enlarging, neighbours read the same dword (a broadcast); shrinking by f, lanes
// are 3 f bytes apart and f = 64 / 3 k columns would put lanes on one bank — the reads are single bytes in a loop
// whose length differs by lane, so the pass is bound by its longest span, not by banks. Its writes and the vertical
// pass's reads are consecutive dwords per lane (e is the low index of both): conflict-free inside one row of sums;
// where a wave straddles two output rows that read different source rows there are two lanes per bank at most.
//
// Matrix instructions are left out: the weights are integers up to 256 per axis (4096 in the product) times bytes, the
// sums must be exact in 32 bits, a box has its own weights (no operand is shared between workgroups), and the kernel
// is bound by the traffic and the colour conversion of staging, not by these multiply-adds.
//
// Not measured: CHIP_ROWS = 8 against 4 or 16, the column chunk of 256, the band of 1024 / sw output rows (which
// fixes 12 accumulators) against smaller bands with more workgroups, byte stores against packed dwords, and the
// occupancy figures above, which are arithmetic, not counters.
// Included by image.hip alone, behind the source tags (enum class Src).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "image_mosaic.h"
#include "image_stage.h"

namespace {
// threads of a workgroup; source rows of a chunk; column groups of a column chunk; dwords of a staged row; accumulators
// of a thread
constexpr int CT = 256, CHIP_ROWS = 8, CHIP_GROUPS = 64, CHIP_ROWW = CHIP_GROUPS * 3 + 1, CHIP_NACC = 12;
constexpr int CHIP_MAX_SIDE = 256, CHIP_MAX_CAPACITY = 256, CHIP_MAX_MARGIN = 64, CHIP_MAX_AREA = 1 << 24;
static_assert(CHIP_ROWW % 2 == 1 && CHIP_GROUPS == 64, "an odd row of dwords; e >> 6 and e & 63 are (row, group)");
static_assert(CHIP_NACC * CT >= 4 * CHIP_MAX_SIDE * 3, "a band of at least four rows of the widest chip");

// The lists and the frame's size as MosaicArgs holds them (cell and mask unused); chips [capacity][sh][sw][3] uint8,
// rows [capacity], rects [capacity][4], chip_count [1] int32; band: output rows of a workgroup, band * sw <= 1024.
struct ChipArgs {
  MosaicArgs m;
  uint8_t* chips;
  int *rows, *rects, *chip_count;
  int capacity, sh, sw, margin, band;
};

// Row r's rectangle, exclusive, grown by the margin and clipped to the frame; false when the rule does not select the
// row or nothing of it is left.
__device__ __forceinline__ bool chip_rect(const ChipArgs& a, int r, int& X0, int& Y0, int& X1, int& Y1) {
  int x0, y0, x1, y1;
  if (!select_rect(a.m, r, x0, y0, x1, y1)) return false;
  X0 = max(x0 - a.margin, 0), Y0 = max(y0 - a.margin, 0);
  X1 = min(x1 + 1 + a.margin, a.m.w), Y1 = min(y1 + 1 + a.margin, a.m.h);
  return X1 > X0 && Y1 > Y0;
}

// Four columns sx .. sx + 3 of row sy of packed pixels of C bytes as a column group: the staging of the patch
// kernel's Src::PACKED3 / PACKED4 for one frame. No byte outside [lo, hi) is read.
template <int C>
__device__ __forceinline__ void stage_packed(const PackedArgs& n, int sy, int sx, uint32_t* dst) {
  uint32_t w[C], px[4];
  load_bytes<4 * C>(w, reinterpret_cast<uintptr_t>(n.s.p) + sy * n.s.pitch + (long long)sx * C, n.s.lo, n.s.hi);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t q;  // pixel k's bytes from bit 0
    if constexpr (C == 4) q = w[k];
    else q = k == 0 ? w[0] : k == 1 ? (w[0] >> 24 | w[1] << 8) : k == 2 ? (w[1] >> 16 | w[2] << 16) : w[2] >> 8;
    px[k] = (q >> (8 * n.r) & 255) | (q >> (8 * n.g) & 255) << 8 | (q >> (8 * n.b) & 255) << 16;
  }
  store_rgb4(dst, px);
}

// The trip counts of the loops that hold barriers (the rows, the chunks) are the same in every thread: n and the
// rectangle are read from LDS, m is summed from LDS; every return is taken by the whole workgroup.
template <Src S, class A, class Y = NoYuv>
__global__ __launch_bounds__(CT) void chips_k(ChipArgs a, A n) {
  extern __shared__ uint32_t c_lds[];
  uint32_t* const s_src = c_lds;                        // [CHIP_ROWS][CHIP_ROWW]: the staged RGB bytes
  uint32_t* const s_h = c_lds + CHIP_ROWS * CHIP_ROWW;  // [CHIP_ROWS][sw][3]: the horizontal sums
  __shared__ int s_wave[CT / 64], s_n, s_rect[5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slot = blockIdx.y, j0 = int(blockIdx.x) * a.band, j1 = min(j0 + a.band, a.sh);
  const int sw = a.sw, sh = a.sh, rows3 = 3 * sw, nout = (j1 - j0) * rows3;
  const bool all = blockIdx.x == 0 && blockIdx.y == 0;
  if (tid == 0) s_n = min(max(a.m.count[0], 0), a.m.N), s_rect[4] = -1;
  __syncthreads();
  const int nrows = s_n;
  int m = 0;  // rows selected so far: the same in every thread
  for (int base = 0; base < nrows && (all || m <= slot); base += CT) {
    const int r = base + tid;
    int x0, y0, x1, y1;
    const bool keep = r < nrows && chip_rect(a, r, x0, y0, x1, y1);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    int off = m;
    for (int k = 0; k < CT / 64; ++k) {
      if (k < wave) off += s_wave[k];
      m += s_wave[k];
    }
    if (keep && off + __popcll(mask & ((1ull << lane) - 1ull)) == slot)
      s_rect[0] = x0, s_rect[1] = y0, s_rect[2] = x1, s_rect[3] = y1, s_rect[4] = r;
    __syncthreads();  // the rectangle is written, and s_wave is free for the next 256 rows
  }
  const int row = s_rect[4];
  if (all && tid == 0) a.chip_count[0] = min(m, a.capacity);
  if (blockIdx.x == 0 && tid < 5) {
    if (tid == 4) a.rows[slot] = row;
    else a.rects[4 * slot + tid] = row < 0 ? 0 : s_rect[tid];
  }
  uint8_t* const out = a.chips + (size_t(slot) * sh + j0) * rows3;
  if (row < 0) {
    for (int e = tid; e < nout; e += CT) out[e] = 0;
    return;
  }
  const int X0 = s_rect[0], Y0 = s_rect[1], X1 = s_rect[2], Y1 = s_rect[3], bw = X1 - X0, bh = Y1 - Y0;
  const uint32_t area = uint32_t(bw) * uint32_t(bh);

  // the vertical pass's outputs: e = tid + CT i is (output row j0 + e / rows3, entry uq = (v, c) of a row of sums);
  // ulo: where the output row starts on the lattice of bh * sh units (far away for an output the band does not have)
  uint32_t acc[CHIP_NACC];
  int ulo[CHIP_NACC], uq[CHIP_NACC];
#pragma unroll
  for (int i = 0; i < CHIP_NACC; ++i) {
    const int e = tid + i * CT, u = e / rows3;
    acc[i] = 0, uq[i] = e < nout ? e - u * rows3 : 0, ulo[i] = e < nout ? (j0 + u) * bh : 1 << 30;
  }
  // the horizontal pass's entries: q = q0 + CT i of staged rows rsub, rsub + rpp, ...; where a row of sums is shorter
  // than the workgroup, rpp rows are summed at a time. hlo: where output column v starts on the lattice of bw * sw
  // units; hs: its first source column; hc: the channel
  int rpp = 1, rsub = 0, q0 = tid;
  if (rows3 < CT) rpp = CT / rows3, rsub = tid / rows3, q0 = rsub < rpp ? tid - rsub * rows3 : rows3;
  int hlo[3], hs[3], hc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int q = min(q0 + i * CT, rows3 - 1), v = q / 3;
    hc[i] = q - 3 * v, hlo[i] = v * bw, hs[i] = hlo[i] / sw;
  }

  const int T0 = j0 * bh / sh, T1 = (j1 * bh + sh - 1) / sh;  // the band's source rows in the rectangle
  const int gx0 = X0 >> 2, ngt = ((X1 - 1) >> 2) - gx0 + 1;   // the rectangle's column groups
  for (int t0 = T0; t0 < T1; t0 += CHIP_ROWS) {
    const int nr = min(CHIP_ROWS, T1 - t0);
    for (int g0 = gx0; g0 < gx0 + ngt; g0 += CHIP_GROUPS) {
      const int ng = min(CHIP_GROUPS, gx0 + ngt - g0);
      for (int e = tid; e < nr * CHIP_GROUPS; e += CT) {
        const int r = e >> 6, g = e & 63;
        if (g >= ng) continue;
        const int sy = Y0 + t0 + r, sx = (g0 + g) * 4;
        uint32_t* dst = s_src + r * CHIP_ROWW + g * 3;
        if constexpr (S == Src::YUV) {
          if constexpr (Y::CHROMA == 1) stage_yuv_bilinear<Y>(n, 0, sy, sx, dst);
          else stage_yuv<Y>(n, 0, sy, sx, dst);
        } else {
          stage_packed<S == Src::PACKED4 ? 4 : 3>(n, sy, sx, dst);
        }
      }
      __syncthreads();
      // the chunk's columns of the rectangle, ca .. cb - 1; column s lies at staged column s + lead
      const int lead = X0 - g0 * 4, ca = max(-lead, 0), cb = min((g0 + ng) * 4 - X0, bw);
      for (int r = rsub; r < nr; r += rpp) {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(s_src + r * CHIP_ROWW);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int q = q0 + i * CT;
          if (q >= rows3) break;
          const int vlo = hlo[i], vhi = vlo + bw;
          uint32_t sum = 0;
          int s = max(hs[i], ca);
          for (int lo = s * sw; s < cb && lo < vhi; ++s, lo += sw)
            sum += uint32_t(min(lo + sw, vhi) - max(lo, vlo)) * src[(s + lead) * 3 + hc[i]];
          uint32_t* hp = s_h + r * rows3 + q;
          *hp = g0 == gx0 ? sum : *hp + sum;
        }
      }
      __syncthreads();  // the sums are written, and the staged rows are free for the next chunk
    }
    for (int r = 0; r < nr; ++r) {
      const int tlo = (t0 + r) * sh;
#pragma unroll
      for (int i = 0; i < CHIP_NACC; ++i) {
        const int wgt = min(tlo + sh, ulo[i] + bh) - max(tlo, ulo[i]);
        if (wgt > 0) acc[i] += uint32_t(wgt) * s_h[r * rows3 + uq[i]];
      }
    }
    // (the next chunk writes the sums behind the barrier that ends its staging: these reads lie before it)
  }
#pragma unroll
  for (int i = 0; i < CHIP_NACC; ++i) {
    const int e = tid + i * CT;
    if (e < nout) out[e] = uint8_t((acc[i] + area / 2) / area);
  }
}
}  // namespace
