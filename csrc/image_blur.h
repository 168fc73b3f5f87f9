// The blur of the image library (image.hip): the detections of selected labels blurred in the frame's own planes by a
// separable Gaussian of integer taps, every painted sample from the frame as it was before the call.
//  * blur_snapshot_k<Surface> — one workgroup of 256 threads per 64 x 64 tile of luma pixels; copies the tiles a
//    blurred box can read to the shadow.
//  * blur_k<Surface> — the same grid; blurs the painted samples of its tile, reading the shadow and writing the frame.
// The rule is exact integers; ops/image.py's blur states it in full.
//
// Why a shadow. The mosaic paints in place because every cell divides its tile; a blurred sample reads `radius` pixels
// past its box, into tiles other workgroups paint. So a call is two launches on one stream. The first copies the frame's
// bytes a blur can read into a shadow buffer the caller brings; the second reads codes from the shadow only and stores
// into the frame only. No workgroup reads a byte another writes: no atomics, no barrier across the grid, no flag, no
// cooperative launch; the order of the two launches on their stream is the only synchronisation. The shadow holds each
// plane of the surface at the plane's own pitch (rows x pitch bytes, image.hip: blur_shadow), so the frame's PackedDst /
// YuvDst with the plane pointers exchanged addresses it, and each shadow plane starts at the plane's address modulo 4,
// so the dword path of stage_rows is taken on both sides alike. Planes one after another, not one span from the first
// plane's first byte to the last plane's last: the planes of a planar surface may be separate allocations.
//
// What is copied. A tile is copied when the rectangle of some selected row, clipped to the frame and grown by the
// radius, touches it. A painted sample (cy, cx) of a box reads codes whose owner pixels lie inside that box grown by the
// radius (the chroma radius is radius >> sub samples, at most radius luma pixels, and a clamped index lies between the
// sample and the unclamped one), so every code that reaches a stored sample was copied. blur_k stages its whole halo,
// which may hold bytes of tiles that were not copied: they are bytes of the shadow, whatever it held, they are masked to
// the surface's depth, and they reach only samples that are not painted, which are not stored.
//
// A workgroup of blur_k:
//  1. Row list, as mosaic_k keeps it: the selected rows whose clipped rectangle touches the tile, four coordinates of
//     0..63 a word. A tile that lists nothing returns before it reads a byte.
//  2. Paint mask: one 64-bit word per row of the tile, bit x set where a listed rectangle covers pixel (y, x). Thread
//     (y, q) ORs the rectangles q, q + 4, ... in registers; four words a row are combined behind a barrier.
//  3. Per colour component, one at a time, and per band of `band` rows of the component's plane (64, or 32 where 64 would
//     not fit: see LDS size): bands and 8-column runs without a painted pixel are skipped.
//     a. Stage. The band plus its halo, (rows + 2 rv) x (cols + 2 rh) samples of the plane's own resolution, as 16-bit
//        codes in LDS. The part inside the plane is walked row by row in dwords (stage_rows of image_mosaic.h), and the
//        clamped indices are resolved here: edge columns, then edge rows, are replicated in LDS behind a barrier each,
//        in edge tiles only. The passes then run without a branch on position.
//     b. Horizontal pass, LDS to LDS. A thread owns a run of 8 adjacent outputs of one row and slides through the
//        8 + 2 rh codes under them once: each code is read once and multiplied into the eight accumulators by the eight
//        taps that apply, which rotate through eight registers (one tap read a code). Taps lie in LDS padded with zeros
//        to a multiple of 8, so a run is whole blocks of 8 x 8 multiply-adds (v_mad_u32_u24: taps <= 256, codes < 2^12,
//        partials < 2^20). Partials are uint16 on 8-bit surfaces (255 * 256 < 2^16) and uint32 on 10 / 12-bit ones.
//     c. Vertical pass. A thread owns a run of 8 adjacent rows of one column and slides down the 8 + 2 rv partials the
//        same way; then the single rounding (sum + 2^15) >> 16, and a store of the samples whose owner pixel is painted.
//  Dst::store writes the three components of a pixel at once, which would keep three components' results in LDS (24 KB);
//  blur_put stores one component's sample with store's own address arithmetic (YuvDst::put, the packed byte).
//
// LDS banks. A wave's lanes in the horizontal pass are 64 consecutive rows at one run, in the vertical pass 64
// consecutive columns at one run. A row of codes is 64 + roundup(2 rh, 8) + 2 halfwords, an odd number of words, so the
// horizontal reads of a wave (one halfword of each of 64 rows at the same column) fall into 64 different banks; a row
// of partials is 66 halfwords (33 words) or 65 words, odd again, so do its writes. The vertical pass reads 64
// consecutive partials of a row: consecutive words, or two lanes a word (one access, broadcast). Tap reads are one
// address a wave. Enumerated on the host for every radius 1..32, both partial types and hsub 0 / 1, the bank of every
// lane of every wave in both passes: no two lanes of a wave share a bank with different words on a 64-bank model, and
// none of a half-wave on a 32-bank model.
//
// LDS size, dynamic: (band + roundup(2 rv, 8)) rows of codes and of partials, as large as the radius needs. Static:
// the list 4 KB, the masks 2.5 KB, taps 0.6 KB. At radius 32 a band of 64 rows takes 33.3 + 16.9 = 50.2 KB on 8-bit
// surfaces (two workgroups a CU) and 66.6 KB on 16-bit ones, above what a workgroup may have; a band of 32 takes 37.6
// and 49.9 KB (three and two workgroups a CU). At radius 16, the default at 1080 rows, 64 rows take 31.5 KB (four).
// The host picks 64 rows where that fits BLUR_BAND_LDS (48 KB: radii up to 28 on 8-bit surfaces, up to 20 on 16-bit
// ones) and 32 otherwise (image.hip: blur_band). Measured as it stands (tools/kbench.py --rows blur, medians of three
// rounds, 400 rows on 2160 x 3840 at radius 32, so bands of 32 rows): NV12 142.5 us, RGB 340.5, P010 205.8 on the whole
// GPU, 909.4, 2311.2 and 1467.7 on 32 CUs; at radius 16 on 1080 x 1920 NV12 (bands of 64) 61.1 and 221.6. Bands of 64
// rows at radius 32 on 8-bit surfaces (50.2 KB, two workgroups a CU, a quarter less halo staged) were not measured.
//
// Matrix instructions were left out. As a banded (Toeplitz) product a pass would be a 64 x 128 by 128 x 64 i8 MFMA
// whose operand is mostly zeros, and neither operand fits i8: taps reach 202 and codes 4095, so each would be split in
// two or three planes of 7 bits and the products recombined, four to six MFMA passes plus the splitting, to replace
// 8 + 2 r multiply-adds an output run. The kernel is bound by staging and LDS traffic, not by its 24-bit multiplies.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see the table behind blur_k.
// Included by image.hip alone, after image_mosaic.h (stage_rows, each_sample, select_rect).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "image_mosaic.h"

namespace {
// threads of a workgroup; the side of its tile; outputs of a run; the largest radius; entries of a tap table on the
// device (2 r + 1 <= 65) and in LDS (roundup(8 + 2 r, 8) <= 72)
constexpr int BT = 256, BTILE = 64, BRUN = 8, BLUR_MAX_RADIUS = 32, BTAPS = 2 * BLUR_MAX_RADIUS + 1, BTAPS_LDS = 80;
// words of a row of uint32 partials, halfwords of a row of uint16 partials
constexpr int BPART32 = 65, BPART16 = 66;
static_assert(BT == MT && BTILE == MTILE, "stage_rows strides by MT; the tile is the mosaic's");
static_assert(BTILE % BRUN == 0 && BT % BTILE == 0 && BPART32 % 2 == 1 && (BPART16 / 2) % 2 == 1, "runs and banks");

// halfwords of a row of codes at axis radius r: the tile, the halo rounded up to whole runs, and two for an odd word count
__host__ __device__ constexpr int blur_code_row(int r) { return BTILE + ((2 * r + 7) & ~7) + 2; }
// rows of codes and partials of a band of `band` rows at axis radius r
__host__ __device__ constexpr int blur_rows(int band, int r) { return band + ((2 * r + 7) & ~7); }
// bytes of dynamic LDS: codes, then partials of pb bytes
__host__ __device__ constexpr int blur_lds(int band, int rh, int rv, int pb) {
  return blur_rows(band, rv) * (blur_code_row(rh) * 2 + (pb == 2 ? BPART16 * 2 : BPART32 * 4));
}

// The lists as MosaicArgs holds them (cell unused); taps: int16 [2][BTAPS] on the device, table s the taps of radius
// >> s; band: 64 or 32 rows.
struct BlurArgs {
  MosaicArgs m;
  const int16_t* taps;
  int radius, band;
};

// ---- one component's sample (cy, cx) stored, with the addresses of PackedDst::store / YuvDst::store ----
__device__ __forceinline__ void blur_put(const PackedDst& d, int comp, int cy, int cx, int code) {
  const int ch = comp == 0 ? d.r : comp == 1 ? 1 : 2 - d.r;
  const_cast<uint8_t*>(d.s.p)[cy * d.s.pitch + (long long)cx * d.C + ch] = uint8_t(code);
}

__device__ __forceinline__ void blur_put(const YuvDst& d, int comp, int cy, int cx, int code) {
  if (d.layout == 2) {
    const int yo = d.order == 1 ? 1 : 0, uo = d.order == 0 ? 1 : d.order == 1 ? 0 : 3, vo = d.order == 0 ? 3 : d.order == 1 ? 2 : 1;
    if (comp == 0) d.put(0, cy, 4LL * (cx >> 1) + yo + 2 * (cx & 1), code);
    else d.put(0, cy, 4LL * cx + (comp == 1 ? uo : vo), code);
  } else if (comp == 0) {
    d.put(0, cy, cx, code);
  } else if (d.layout == 1) {
    d.put(1, cy, 2LL * cx + (comp == 1 ? d.order : 1 - d.order), code);
  } else {
    d.put(comp, cy, cx, code);
  }
}

__device__ __forceinline__ bool blur_wide(const PackedDst&) { return false; }
__device__ __forceinline__ bool blur_wide(const YuvDst& d) { return d.sb == 2; }

// Component comp's samples (gy0 .. gy0 + rows - 1) x (gx0 .. gx0 + cols - 1) of its plane, all inside the plane, as
// codes: sample (gy0 + i, gx0 + j) at code[i * cs + j]. No byte outside those rows' bytes of the plane is read (of a
// YUY2 row: outside the macropixels that hold them, which lie inside the row).
__device__ __forceinline__ void blur_stage(const PackedDst& d, int, int comp, int gy0, int gx0, int rows, int cols,
                                           uint16_t* code, int cs) {
  const int C = d.C, ch = comp == 0 ? d.r : comp == 1 ? 1 : 2 - d.r;
  stage_rows(d.s.p + gy0 * d.s.pitch + (long long)gx0 * C, d.s.pitch, rows, cols * C, [=](int row, int b, uint32_t v, int n) {
    for (int k = 0; k < n; ++k) {
      const int at = b + k, px = C == 4 ? at >> 2 : at / 3;
      if (at - px * C == ch) code[row * cs + px] = uint16_t((v >> (8 * k)) & 255u);
    }
  });
}

__device__ __forceinline__ void blur_stage(const YuvDst& d, int mask, int comp, int gy0, int gx0, int rows, int cols,
                                           uint16_t* code, int cs) {
  const int sb = d.sb, shift = d.shift, order = d.order;
  if (d.layout == 2) {
    const int yo = order == 1 ? 1 : 0, uo = order == 0 ? 1 : order == 1 ? 0 : 3, vo = order == 0 ? 3 : order == 1 ? 2 : 1;
    if (comp == 0) {
      // the macropixels of luma gx0 .. gx0 + cols - 1; a luma sample outside that range is dropped
      const int mp0 = gx0 >> 1, mps = ((gx0 + cols - 1) >> 1) - mp0 + 1;
      stage_rows(d.pl[0].p + gy0 * d.pl[0].pitch + 4LL * mp0, d.pl[0].pitch, rows, 4 * mps,
                 [=](int row, int b, uint32_t v, int n) {
                   for (int k = 0; k < n; ++k) {
                     const int at = b + k, pos = (at & 3) - yo;
                     const int j = 2 * (mp0 + (at >> 2)) + (pos >> 1) - gx0;
                     if ((pos == 0 || pos == 2) && j >= 0 && j < cols) code[row * cs + j] = uint16_t((v >> (8 * k)) & 255u);
                   }
                 });
    } else {
      const int want = comp == 1 ? uo : vo;
      stage_rows(d.pl[0].p + gy0 * d.pl[0].pitch + 4LL * gx0, d.pl[0].pitch, rows, 4 * cols,
                 [=](int row, int b, uint32_t v, int n) {
                   for (int k = 0; k < n; ++k)
                     if (((b + k) & 3) == want) code[row * cs + ((b + k) >> 2)] = uint16_t((v >> (8 * k)) & 255u);
                 });
    }
    return;
  }
  if (comp == 0 || d.layout == 0) {
    const PlaneArg& q = d.pl[comp];
    stage_rows(q.p + gy0 * q.pitch + (long long)gx0 * sb, q.pitch, rows, cols * sb, [=](int row, int b, uint32_t v, int n) {
      each_sample(sb, shift, mask, b, v, n, [=](int e, int c) { code[row * cs + e] = uint16_t(c); });
    });
    return;
  }
  // pairs: U at sample 2 cx + order
  const int want = comp == 1 ? order : 1 - order;
  stage_rows(d.pl[1].p + gy0 * d.pl[1].pitch + 2LL * gx0 * sb, d.pl[1].pitch, rows, 2 * cols * sb,
             [=](int row, int b, uint32_t v, int n) {
               each_sample(sb, shift, mask, b, v, n, [=](int e, int c) {
                 if ((e & 1) == want) code[row * cs + (e >> 1)] = uint16_t(c);
               });
             });
}

// The tile's in-frame bytes of every plane, from the frame's planes to the shadow's (the same pitches, the same
// addresses modulo 4): dwords where stage_rows loaded one, bytes otherwise.
__device__ __forceinline__ void blur_copy(const uint8_t* from, uint8_t* to, long long pitch, int rows, int bytes) {
  stage_rows(from, pitch, rows, bytes, [=](int row, int b, uint32_t v, int n) {
    uint8_t* q = to + row * pitch + b;
    if (n == 4 && (reinterpret_cast<uintptr_t>(q) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(q) = v;
    } else {
      for (int k = 0; k < n; ++k) q[k] = uint8_t(v >> (8 * k));
    }
  });
}

__device__ __forceinline__ void blur_snapshot(const PackedDst& d, const PackedDst& s, int ty0, int tx0, int th, int tw) {
  const long long at = ty0 * d.s.pitch + (long long)tx0 * d.C;
  blur_copy(d.s.p + at, const_cast<uint8_t*>(s.s.p) + at, d.s.pitch, th, tw * d.C);
}

__device__ __forceinline__ void blur_snapshot(const YuvDst& d, const YuvDst& s, int ty0, int tx0, int th, int tw) {
  const int sb = d.sb;
  if (d.layout == 2) {
    const long long at = ty0 * d.pl[0].pitch + 2LL * tx0;
    blur_copy(d.pl[0].p + at, const_cast<uint8_t*>(s.pl[0].p) + at, d.pl[0].pitch, th, 4 * ((tw + 1) >> 1));
    return;
  }
  const long long at = ty0 * d.pl[0].pitch + (long long)tx0 * sb;
  blur_copy(d.pl[0].p + at, const_cast<uint8_t*>(s.pl[0].p) + at, d.pl[0].pitch, th, tw * sb);
  const int cy0 = ty0 >> d.vsub, cx0 = tx0 >> d.hsub;
  const int tch = (th + (1 << d.vsub) - 1) >> d.vsub, tcw = (tw + (1 << d.hsub) - 1) >> d.hsub;
  const int np = d.layout == 1 ? 2 : 3, per = d.layout == 1 ? 2 * sb : sb;  // bytes of a chroma column of a plane
  for (int i = 1; i < np; ++i) {
    const long long c = cy0 * d.pl[i].pitch + (long long)cx0 * per;
    blur_copy(d.pl[i].p + c, const_cast<uint8_t*>(s.pl[i].p) + c, d.pl[i].pitch, tch, tcw * per);
  }
}

// Every return is taken by the whole workgroup: the vote is a barrier all threads reach.
template <class Dst>
__global__ __launch_bounds__(BT) void blur_snapshot_k(BlurArgs b, Dst dst, Dst shadow) {
  const MosaicArgs& a = b.m;
  const int tiles_x = (a.w + BTILE - 1) / BTILE;
  const int ty0 = int(blockIdx.x) / tiles_x * BTILE, tx0 = int(blockIdx.x) % tiles_x * BTILE;
  const int th = min(BTILE, a.h - ty0), tw = min(BTILE, a.w - tx0);
  const int n = min(max(a.count[0], 0), a.N);
  int hit = 0;
  for (int r = threadIdx.x; r < n && !hit; r += BT) {
    int x0, y0, x1, y1;
    if (!select_rect(a, r, x0, y0, x1, y1)) continue;
    x0 = max(x0, 0), y0 = max(y0, 0), x1 = min(x1, a.w - 1), y1 = min(y1, a.h - 1);
    if (x0 > x1 || y0 > y1) continue;
    hit = x0 - b.radius < tx0 + tw && x1 + b.radius >= tx0 && y0 - b.radius < ty0 + th && y1 + b.radius >= ty0;
  }
  if (!__syncthreads_or(hit)) return;
  blur_snapshot(dst, shadow, ty0, tx0, th, tw);
}

// One pass of a band. P: the partials' type. code: rows x cs halfwords; part: rows x ps of P; s_tap: the two padded
// tables; colmask: the columns of the tile with a painted pixel in the band.
template <class P, class Dst>
__device__ __forceinline__ void blur_band(const Dst& dst, const uint16_t* code, P* part, int cs, int ps, const int* tap_h,
                                          const int* tap_v, int rh, int rv, int comp, int hs, int vs, int cy0, int cx0,
                                          int by, int brows, int tcw, const unsigned long long* s_paint,
                                          unsigned long long colmask) {
  const int tid = threadIdx.x;
  const int nh = BRUN + ((2 * rh + 7) & ~7), nv = BRUN + ((2 * rv + 7) & ~7);  // codes under a run, zero taps included
  const int rrows = brows + 2 * rv;
  // horizontal: item i is row (i >> 9) * 64 + (i & 63), run (i >> 6) & 7
  for (int i = tid; i < ((rrows + 63) >> 6) << 9; i += BT) {
    const int row = ((i >> 9) << 6) + (i & 63), run = (i >> 6) & 7;
    if (row >= rrows || run * BRUN >= tcw) continue;
    const int bit = (run * BRUN) << hs;
    if (((colmask >> bit) & ((hs ? 0xffffull : 0xffull))) == 0) continue;
    const uint16_t* q = code + row * cs + run * BRUN;
    int acc[BRUN] = {}, w[BRUN] = {};
    for (int k0 = 0; k0 < nh; k0 += BRUN) {
#pragma unroll
      for (int kk = 0; kk < BRUN; ++kk) {
        w[kk] = tap_h[k0 + kk];
        const int c = q[k0 + kk];
#pragma unroll
        for (int o = 0; o < BRUN; ++o) acc[o] += __mul24(w[(kk - o) & (BRUN - 1)], c);
      }
    }
#pragma unroll
    for (int o = 0; o < BRUN; ++o) part[row * ps + run * BRUN + o] = P(acc[o]);
  }
  __syncthreads();
  // vertical: item i is column i & 63, run i >> 6; the outputs are rows run * 8 .. + 7 of the band
  for (int i = tid; i < ((brows + BRUN - 1) / BRUN) << 6; i += BT) {
    const int col = i & 63, run = i >> 6;
    if (col >= tcw) continue;
    const int lx = col << hs, ly0 = (by + run * BRUN - cy0) << vs;  // the owner pixel of output 0, in the tile
    unsigned on = 0;
#pragma unroll
    for (int o = 0; o < BRUN; ++o)
      if (run * BRUN + o < brows) on |= unsigned((s_paint[ly0 + (o << vs)] >> lx) & 1ull) << o;
    if (on == 0) continue;
    const P* q = part + run * BRUN * ps + col;
    int acc[BRUN] = {}, w[BRUN] = {};
    for (int k0 = 0; k0 < nv; k0 += BRUN) {
#pragma unroll
      for (int kk = 0; kk < BRUN; ++kk) {
        w[kk] = tap_v[k0 + kk];
        const int c = int(q[(k0 + kk) * ps]);
#pragma unroll
        for (int o = 0; o < BRUN; ++o) acc[o] += __mul24(w[(kk - o) & (BRUN - 1)], c);
      }
    }
#pragma unroll
    for (int o = 0; o < BRUN; ++o)
      if ((on >> o) & 1u) blur_put(dst, comp, by + run * BRUN + o, cx0 + col, (acc[o] + (1 << 15)) >> 16);
  }
}

// The trip count of every loop that holds a barrier is read from LDS or from the arguments by all threads, and every
// return and every skipped band is taken by the whole workgroup.
// Resource usage, gfx950 (the compiler's remarks; scratch 0 in all four, SGPR spills go to VGPR lanes):
//   blur_k<PackedDst>           VGPR  68  SGPR 106 (11 spilled)   static LDS 7328 B  scratch 0  7 waves/SIMD
//   blur_k<YuvDst>              VGPR 124  SGPR 106 (138 spilled)  static LDS 7328 B  scratch 0  4 waves/SIMD
//   blur_snapshot_k<PackedDst>  VGPR  16  SGPR  68                static LDS  256 B  scratch 0  8 waves/SIMD
//   blur_snapshot_k<YuvDst>     VGPR  20  SGPR  62                static LDS  256 B  scratch 0  8 waves/SIMD
// The dynamic LDS, not the registers, bounds the workgroups of blur_k on a CU: four waves a SIMD are four workgroups.
template <class Dst>
__global__ __launch_bounds__(BT) void blur_k(BlurArgs b, Dst dst, Dst shadow) {
  extern __shared__ __align__(16) uint8_t s_dyn[];
  __shared__ uint32_t s_rect[OMAX];
  __shared__ unsigned long long s_paint[BTILE], s_pm[BT];
  __shared__ int s_tap[2][BTAPS_LDS];
  __shared__ int s_wave[BT / 64], s_n;
  const MosaicArgs& a = b.m;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (a.w + BTILE - 1) / BTILE;
  const int ty0 = int(blockIdx.x) / tiles_x * BTILE, tx0 = int(blockIdx.x) % tiles_x * BTILE;
  const int th = min(BTILE, a.h - ty0), tw = min(BTILE, a.w - tx0);  // the tile's pixels inside the frame
  if (tid == 0) s_n = min(max(a.count[0], 0), a.N);
  if (tid < 2 * BTAPS_LDS) {
    const int t = tid / BTAPS_LDS, j = tid - t * BTAPS_LDS;
    s_tap[t][j] = j <= 2 * (b.radius >> t) ? int(b.taps[t * BTAPS + j]) : 0;
  }
  __syncthreads();
  const int n = s_n;
  int m = 0;  // rows listed so far: the same in every thread
  for (int base = 0; base < n; base += BT) {
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
    for (int k = 0; k < BT / 64; ++k) {
      if (k < wave) off += s_wave[k];
      m += s_wave[k];
    }
    if (keep) s_rect[off + __popcll(mask & ((1ull << lane) - 1ull))] = uint32_t(x0 | x1 << 8 | y0 << 16 | y1 << 24);
    __syncthreads();  // the list is written, and s_wave is free for the next 256 rows
  }
  if (m == 0) return;

  // the paint mask: thread (y = lane, q = wave) ORs the rectangles q, q + 4, ...
  {
    unsigned long long bits = 0;
    for (int i = wave; i < m; i += BT / 64) {
      const uint32_t q = s_rect[i];
      const int x0 = q & 255, x1 = (q >> 8) & 255, y0 = (q >> 16) & 255, y1 = q >> 24;
      if (lane >= y0 && lane <= y1) bits |= (~0ull >> (63 - (x1 - x0))) << x0;
    }
    s_pm[tid] = bits;
    __syncthreads();
    if (tid < BTILE) s_paint[tid] = s_pm[tid] | s_pm[tid + 64] | s_pm[tid + 128] | s_pm[tid + 192];
    __syncthreads();
  }

  int hsub, vsub;
  mosaic_sub(dst, hsub, vsub);
  const bool wide = blur_wide(dst);
  for (int comp = 0; comp < 3; ++comp) {
    const int hs = comp ? hsub : 0, vs = comp ? vsub : 0;
    const int rh = b.radius >> hs, rv = b.radius >> vs;
    const int ph = (a.h + (1 << vs) - 1) >> vs, pw = (a.w + (1 << hs) - 1) >> hs;  // the plane
    const int cy0 = ty0 >> vs, cx0 = tx0 >> hs;
    const int tch = (th + (1 << vs) - 1) >> vs, tcw = (tw + (1 << hs) - 1) >> hs;  // the tile's samples
    const int cs = blur_code_row(rh), ps = wide ? BPART32 : BPART16;
    uint16_t* const code = reinterpret_cast<uint16_t*>(s_dyn);
    uint8_t* const part = s_dyn + blur_rows(b.band, rv) * cs * 2;
    for (int b0 = 0; b0 < tch; b0 += b.band) {
      const int brows = min(b.band, tch - b0), by = cy0 + b0;
      unsigned long long colmask = 0;
      for (int y = b0 << vs; y < min((b0 + brows) << vs, th); ++y) colmask |= s_paint[y];
      if (colmask == 0) continue;
      // the region: rows by - rv .. by + brows - 1 + rv, columns cx0 - rh .. cx0 + tcw - 1 + rh; inside the plane:
      const int gy_lo = max(by - rv, 0), gy_hi = min(by + brows - 1 + rv, ph - 1);
      const int gx_lo = max(cx0 - rh, 0), gx_hi = min(cx0 + tcw - 1 + rh, pw - 1);
      const int top = gy_lo - (by - rv), left = gx_lo - (cx0 - rh);  // the first staged row and column of the region
      const int rrows = brows + 2 * rv, rcols = tcw + 2 * rh;
      const int nrow = gy_hi - gy_lo + 1, ncol = gx_hi - gx_lo + 1;
      blur_stage(shadow, a.mask, comp, gy_lo, gx_lo, nrow, ncol, code + top * cs + left, cs);
      if (ncol < rcols) {  // edge columns, in the staged rows
        __syncthreads();
        const int miss = rcols - ncol;
        for (int i = tid; i < nrow * miss; i += BT) {
          const int row = top + i / miss, j = i % miss, col = j < left ? j : ncol + j;
          code[row * cs + col] = code[row * cs + (j < left ? left : left + ncol - 1)];
        }
      }
      if (nrow < rrows) {  // edge rows, whole
        __syncthreads();
        const int miss = rrows - nrow;
        for (int i = tid; i < miss * rcols; i += BT) {
          const int j = i / rcols, col = i - j * rcols, row = j < top ? j : nrow + j;
          code[row * cs + col] = code[(j < top ? top : top + nrow - 1) * cs + col];
        }
      }
      __syncthreads();
      if (wide)
        blur_band(dst, code, reinterpret_cast<uint32_t*>(part), cs, ps, s_tap[hs], s_tap[vs], rh, rv, comp, hs, vs, cy0,
                  cx0, by, brows, tcw, s_paint, colmask);
      else
        blur_band(dst, code, reinterpret_cast<uint16_t*>(part), cs, ps, s_tap[hs], s_tap[vs], rh, rv, comp, hs, vs, cy0,
                  cx0, by, brows, tcw, s_paint, colmask);
      __syncthreads();  // the codes and partials are free for the next band
    }
  }
}
}  // namespace
