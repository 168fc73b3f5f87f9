// The converter of the image library (image.hip): a frame of any source the chips read — packed pixels, any YUV layout
// with nearest or bilinear chroma, PQ / HLG through the tables — written into a second surface of any SDR layout, depth,
// subsampling and order at any size. The read side is the chips' (image_stage.h, stage_packed), the rule of the resize
// is theirs too (the exact area average of the converted frame); what is new is the forward colour rule and the kernel
// between the two.
//  * convert_k<Src, source arguments, Yuv<...>, SAME> — one launch; the rule is exact integers, ops/image.py's convert
//    states it in full. The source's layout is the instantiation (the chips' table, yuv_dispatch), the target's is a
//    runtime description (ConvPlane), so there are twice the chips' instantiations and not their product with the
//    target layouts.
//
// How the work is split. The grid is a flat list of tiles of the *target*: CV_TW = 128 luma columns x a band of rows.
// The band is CV_BAND = 8 rows, halved by the host (down to 2) while the grid would hold fewer than 1024 workgroups. Tile
// origins are even in both axes, so a chroma block (1, 2 or 4 luma pixels) lies inside one tile and no two workgroups
// write the same storage unit. The grid depends on the two sizes alone.
//
// Phase 1, resampling (SAME = false). The tile's source footprint — rows floor(J0 h / H) .. ceil(J1 h / H) - 1 and the
// column groups under columns floor(I0 w / W) .. ceil(I1 w / W) - 1 — is streamed through LDS in chunks of CV_ROWS = 8
// rows x CV_GROUPS = 64 column groups (256 columns). A column group is four columns of the *frame*, so a chroma pair lies
// under its luma; thread (row, group) stages it as 12 RGB bytes with the read side's functions. Thread (v, half) owns
// output column I0 + v and half of the band's rows (the upper half in waves 0 and 1, the lower in waves 2 and 3), three
// channels each: CV_NACC = 12 accumulators. Horizontal pass: for every staged row that overlaps the thread's rows (a
// wave-uniform test: shrinking, the two halves read disjoint rows but for a seam) it sums, per channel, overlap x byte
// over the source columns its column overlaps inside the chunk, in 32-bit registers. Vertical pass, fused: the three
// sums go straight into the accumulators times the row's overlap with each output row, so no sum touches LDS and a
// column chunk just adds its part. All weights are lattice arithmetic (min / max of multiples of the four sizes); there
// are no tables. One unsigned division per output, (sum + A / 2) / A with A = h w <= 2^24 (the entry refuses more), so
// sum + A / 2 < 2^32. The pixel goes to the LDS tile s_rgb [8][128] as R | G << 8 | B << 16.
//
// Phase 1, SAME = true. At equal sizes the staged bytes are the tile: thread (row, group) stages one group of the tile's
// 8 x 32, and phase 2 reads the pixels out of the staged rows. No sums, no division, no second buffer, no limit on the
// frame's area.
//
// Phase 2, behind one barrier. For each storage plane of the target the tile is a list of *store units* of U
// consecutive slots of a row (a slot: one sample, a byte or a 16-bit word; a row is periods of P slots, ConvPlane::slots
// says what each slot of a period holds): U = 4 for 8-bit planar samples and for a YUY2 macropixel, 2 for a UV pair, 1
// for a 16-bit planar sample and for the bytes of a packed pixel. Thread e takes unit e, e + 256, ...: consecutive lanes
// store consecutive addresses. It computes the unit's codes — a colour byte of the pixel; luma from the pixel; chroma
// from the sum of the block's 1, 2 or 4 pixels clipped to the frame, summed once per period — with the 12 integers of
// convert_table (2^-14 fixed point; at depth 12 every coefficient is below 2^18 in size, a row's absolute sum below
// 2^18.1, and with S <= 1020 per channel and the offset term below 2^27.1 every sum stays below 2^29: int32). A unit
// all of whose slots are samples of the frame, at an address that is a multiple of its size, is one store of 2 or 4
// bytes; any other unit — an unaligned surface, the half-filled last macropixel of an odd width, the last samples of a
// row — is stored sample by sample. The fourth byte of RGBA / BGRA is a slot of no component and is never written.
//
// LDS: CV_ROWS x CV_ROWW dwords staged = 6.0 KB, and without SAME the 4 KB of s_rgb: 10.0 KB a workgroup, static: 26
// and 15 workgroups a CU by LDS, so the waves bind first. Banks. Staging: lanes are consecutive groups of a row, 3 dwords apart, coprime to the bank
// count: conflict-free; a staged row is CV_ROWW = 193 dwords (odd), so rows start in different banks. Horizontal pass:
// lanes are consecutive output columns; enlarging, neighbours read the same bytes (a broadcast); shrinking by f they
// read bytes 3 f apart in a loop whose length differs by at most one between lanes. s_rgb: lanes write and read
// consecutive dwords; a chroma unit reads two columns of two rows, lanes two dwords apart: two lanes a bank. SAME:
// phase 2 reads bytes 3 apart across lanes, 48 dwords a wave: conflict-free.
//
// Registers: the compiler reports, by instantiation, 28 to 42 VGPRs (SAME) and 51 to 79 (resampling) — the most for
// bilinear chroma, whose staging holds two chroma windows — and no scratch in any of the 44; 8 waves a SIMD with SAME,
// 6 to 8 resampling.
//
// Matrix instructions are left out: the resample's weights differ per output column and row and its sums must be exact
// integers of up to 32 bits; the colour rule is a 3 x 3 integer product per pixel with an arithmetic shift and a clip,
// whose operands (8-bit pixels, 18-bit coefficients) no MFMA format holds exactly.
//
// Not measured against their alternatives: the tile of 128 x 8 against 256 x 4 or 64 x 16, the band rule, the two
// halves of a band per column against a thread per (column, channel), the fused vertical pass against sums kept in
// LDS as the chips keep them, a unit per thread against rescale_k's sample per thread with shuffles, the runtime
// target description against an instantiation per target layout, dword stores against wider ones, and for a
// four-byte pixel (the slowest target measured) a 16-bit store of two colour bytes against three single bytes. What binds the
// kernel was not measured with counters either; ops/image.py's convert names the figures that were.
// Included by image.hip alone, behind image_chips.h (Src, stage_packed).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "image_stage.h"

namespace {
// threads of a workgroup; columns of a tile; rows of a band at most; source rows and column groups of a chunk; dwords
// of a staged row; accumulators of a thread; the largest side; the largest source of the resampling path
constexpr int CV_T = 256, CV_TW = 128, CV_BAND = 8, CV_ROWS = 8, CV_GROUPS = 64, CV_ROWW = CV_GROUPS * 3 + 1;
constexpr int CV_NACC = 12, CV_MAX_SIDE = 8192, CV_MAX_AREA = 1 << 24;
static_assert(CV_ROWW % 2 == 1 && CV_GROUPS == 64, "an odd row of dwords; e >> 6 and e & 63 are (row, group)");
static_assert(CV_T == 2 * CV_TW && CV_NACC == 3 * CV_BAND / 2, "a thread per column and half of the band");
static_assert(CV_BAND <= CV_ROWS && CV_TW / 4 * CV_BAND == CV_T, "SAME: the tile is one chunk, a group a thread");

// What a slot of a period holds: nothing; channel `arg` of the pixel (packed targets); the luma of the period's column
// `arg`; U or V of the period's block. A byte per slot in ConvPlane::slots, kind | arg << 3.
enum { CV_NONE = 0, CV_BYTE = 1, CV_LUMA = 2, CV_U = 3, CV_V = 4 };

// One storage plane of the target: a row is periods of P slots, a period covers 1 << cs luma columns and a row 1 << vs
// luma rows; unit: the slots of a store unit (1, 2 or 4; unit * sample bytes <= 4, and P and unit divide one another).
struct ConvPlane {
  uint8_t* p;
  long long pitch;
  uint32_t slots;
  int P, cs, vs, unit;
};

// The target (np planes; sb bytes a sample, stored as code << shift, codes clipped to maxcode; tab: convert_table's 12
// integers, unused by a packed target), the two sizes, and the grid: band rows a tile, tiles_x tiles a row of tiles.
struct ConvArgs {
  ConvPlane pl[3];
  int tab[12];
  int np, sb, shift, maxcode;
  int h, w, H, W;
  int band, tiles_x;
};

// clip((t . s + (off << (14 + k)) + (1 << (13 + k))) >> (14 + k), 0, maxcode): row `row` of the table on the sum s of
// 1 << k pixels
__device__ __forceinline__ int convert_code(const int* tab, int row, const int (&s)[3], int k, int maxcode) {
  const int* t = tab + 3 * row;
  const int v = t[0] * s[0] + t[1] * s[1] + t[2] * s[2] + (tab[9 + row] << (14 + k)) + (1 << (13 + k));
  return min(max(v >> (14 + k), 0), maxcode);
}

// The trip counts of the loops that hold barriers (the row chunks, the column chunks) come from the kernel's arguments
// and the workgroup's index alone.
template <Src S, class A, class Y, bool SAME>
__global__ __launch_bounds__(CV_T) void convert_k(ConvArgs a, A n) {
  __shared__ uint32_t s_src[CV_ROWS * CV_ROWW];            // the staged RGB bytes
  __shared__ uint32_t s_rgb[SAME ? 1 : CV_BAND * CV_TW];   // the resampled tile, R | G << 8 | B << 16
  const int tid = threadIdx.x;
  const int ty = int(blockIdx.x) / a.tiles_x, tx = int(blockIdx.x) - ty * a.tiles_x;
  const int I0 = tx * CV_TW, I1 = min(I0 + CV_TW, a.W), J0 = ty * a.band, J1 = min(J0 + a.band, a.H);

  // four columns sx .. sx + 3 of source row sy as a column group
  auto stage = [&](int sy, int sx, uint32_t* dst) {
    if constexpr (S == Src::YUV) {
      if constexpr (Y::CHROMA == 1) stage_yuv_bilinear<Y>(n, 0, sy, sx, dst);
      else stage_yuv<Y>(n, 0, sy, sx, dst);
    } else {
      stage_packed<S == Src::PACKED4 ? 4 : 3>(n, sy, sx, dst);
    }
  };

  if constexpr (SAME) {
    const int r = tid >> 5, g = tid & 31, sx = I0 + 4 * g;
    if (J0 + r < J1 && sx < I1) stage(J0 + r, sx, s_src + r * CV_ROWW + 3 * g);
  } else {
    const int h = a.h, w = a.w, H = a.H, W = a.W;
    // the thread's column and rows; on the lattice of w * W units its column is [vlo, vhi), source column s is
    // [s W, (s + 1) W), and likewise for the rows with h and H
    const int v = tid & (CV_TW - 1), hb = a.band >> 1, Ja = J0 + (tid >> 7) * hb, Jb = min(Ja + hb, J1);
    const bool active = I0 + v < I1 && Ja < Jb;
    const int vlo = (I0 + v) * w, vhi = vlo + w, hs = vlo / W;
    uint32_t acc[CV_NACC];
#pragma unroll
    for (int i = 0; i < CV_NACC; ++i) acc[i] = 0;
    const int T0 = J0 * h / H, T1 = (J1 * h + H - 1) / H;  // the band's source rows
    const int gx0 = (I0 * w / W) >> 2, gx1 = (((I1 * w + W - 1) / W - 1) >> 2) + 1;  // the tile's column groups
    for (int t0 = T0; t0 < T1; t0 += CV_ROWS) {
      const int nr = min(CV_ROWS, T1 - t0);
      for (int g0 = gx0; g0 < gx1; g0 += CV_GROUPS) {
        const int ng = min(CV_GROUPS, gx1 - g0);
        __syncthreads();  // the last chunk's reads lie before this barrier
        for (int e = tid; e < nr * CV_GROUPS; e += CV_T) {
          const int r = e >> 6, g = e & 63;
          if (g < ng) stage(t0 + r, (g0 + g) * 4, s_src + r * CV_ROWW + 3 * g);
        }
        __syncthreads();
        if (!active) continue;
        // the chunk's columns the thread's column overlaps
        const int ca = max(hs, g0 * 4), cb = min((g0 + ng) * 4, w);
        for (int r = 0; r < nr; ++r) {
          const int tlo = (t0 + r) * H;
          if (tlo + H <= Ja * h || tlo >= Jb * h) continue;  // (the same in every lane of a wave)
          const uint8_t* const src = reinterpret_cast<const uint8_t*>(s_src + r * CV_ROWW);
          uint32_t sum[3] = {0, 0, 0};
          for (int s = ca, lo = ca * W; s < cb && lo < vhi; ++s, lo += W) {
            const uint32_t wgt = uint32_t(min(lo + W, vhi) - max(lo, vlo));
            const uint8_t* const px = src + 3 * (s - 4 * g0);
            sum[0] += wgt * px[0], sum[1] += wgt * px[1], sum[2] += wgt * px[2];
          }
#pragma unroll
          for (int i = 0; i < CV_BAND / 2; ++i) {
            const int ulo = (Ja + i) * h, wgt = min(tlo + H, ulo + h) - max(tlo, ulo);
            if (Ja + i < Jb && wgt > 0) {
#pragma unroll
              for (int c = 0; c < 3; ++c) acc[3 * i + c] += uint32_t(wgt) * sum[c];
            }
          }
        }
      }
    }
    const uint32_t area = uint32_t(h) * uint32_t(w);
#pragma unroll
    for (int i = 0; i < CV_BAND / 2; ++i) {
      if (active && Ja + i < Jb)
        s_rgb[(Ja + i - J0) * CV_TW + v] = (acc[3 * i] + area / 2) / area | (acc[3 * i + 1] + area / 2) / area << 8 |
                                           (acc[3 * i + 2] + area / 2) / area << 16;
    }
  }
  __syncthreads();

  // pixel (r, x) of the tile as R | G << 8 | B << 16
  auto pixel = [&](int r, int x) -> uint32_t {
    if constexpr (SAME) {
      const uint8_t* const q = reinterpret_cast<const uint8_t*>(s_src + r * CV_ROWW) + 3 * x;
      return uint32_t(q[0]) | uint32_t(q[1]) << 8 | uint32_t(q[2]) << 16;
    } else {
      return s_rgb[r * CV_TW + x];
    }
  };

  const int sb = a.sb, ncol = I1 - I0, nrow = J1 - J0;
  for (int q = 0; q < a.np; ++q) {
    const ConvPlane& p = a.pl[q];
    const int P = p.P, cs = p.cs, vs = p.vs, U = p.unit;
    const int nslot = ((ncol + (1 << cs) - 1) >> cs) * P, upr = (nslot + U - 1) / U;  // slots and units of a row
    const int rows = (nrow + (1 << vs) - 1) >> vs;
    for (int e = tid; e < rows * upr; e += CV_T) {
      const int row = e / upr, slot0 = (e - row * upr) * U;
      uint8_t* const at = p.p + (long long)((J0 >> vs) + row) * p.pitch + ((long long)(I0 >> cs) * P + slot0) * sb;
      uint32_t word = 0, valid = 0;  // the unit's samples from bit 0, and which of them are samples of the frame
      int block = -1, k = 0, sum[3];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int slot = slot0 + j;
        if (j >= U || slot >= nslot) break;
        const int per = slot / P;
        const uint32_t info = (p.slots >> (8 * (slot - per * P))) & 255u;
        const int kind = int(info & 7u), arg = int(info >> 3);
        int code;
        if (kind == CV_NONE) continue;
        if (kind == CV_BYTE || kind == CV_LUMA) {
          // (these planes have vs = 0: the plane's row is the tile's)
          const int x = (per << cs) + (kind == CV_LUMA ? arg : 0);
          if (x >= ncol) continue;
          const uint32_t px = pixel(row, x);
          if (kind == CV_BYTE) {
            code = int((px >> (8 * arg)) & 255u);
          } else {
            const int s[3] = {int(px & 255u), int((px >> 8) & 255u), int(px >> 16)};
            code = convert_code(a.tab, 0, s, 0, a.maxcode);
          }
        } else {
          if (block != per) {
            // the block's pixels inside the frame: 1, 2 or 4 of them
            const int r0 = row << vs, r1 = min(r0 + (1 << vs), nrow), x0 = per << cs, x1 = min(x0 + (1 << cs), ncol);
            sum[0] = sum[1] = sum[2] = 0;
            for (int r = r0; r < r1; ++r)
              for (int x = x0; x < x1; ++x) {
                const uint32_t px = pixel(r, x);
                sum[0] += int(px & 255u), sum[1] += int((px >> 8) & 255u), sum[2] += int(px >> 16);
              }
            block = per, k = ((r1 - r0) * (x1 - x0)) >> 1;  // log2 of 1, 2, 4
          }
          code = convert_code(a.tab, kind == CV_U ? 1 : 2, sum, k, a.maxcode);
        }
        word |= uint32_t(code << a.shift) << (8 * sb * j), valid |= 1u << j;
      }
      const int bytes = U * sb;
      if (valid == (1u << U) - 1u && (reinterpret_cast<uintptr_t>(at) & uintptr_t(bytes - 1)) == 0) {
        if (bytes == 4) *reinterpret_cast<uint32_t*>(at) = word;
        else if (bytes == 2) *reinterpret_cast<uint16_t*>(at) = uint16_t(word);
        else *at = uint8_t(word);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!((valid >> j) & 1u)) continue;
          if (sb == 2) *reinterpret_cast<uint16_t*>(at + 2 * j) = uint16_t(word >> (16 * j));
          else at[j] = uint8_t(word >> (8 * j));
        }
      }
    }
  }
}
}  // namespace
