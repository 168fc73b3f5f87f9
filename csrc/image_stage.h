// Staging for the image kernel (image.hip): everything that turns a source into the RGB bytes of the LDS tile.
//  * the argument structs a source's staging loop reads (one per layout, Tiled<A> for B tiles of one frame) and the
//    Yuv<layout, hsub, sample bytes, chroma> tags the general YUV front end is instantiated by;
//  * the reads: load4 (four bytes, those inside the storage), load_bytes (any count at any alignment);
//  * the colour functions: nv12_channel / yuv_to_rgb4 (8-bit 4:2:0), yuv_channel (any depth), hdr_pixel (PQ / HLG
//    through the tables);
//  * stage_yuv (nearest chroma) and stage_yuv_bilinear (chroma_window, chroma_row4): four columns of a YUV source
//    as one column group, 12 RGB bytes written by store_rgb4.
// Included by image.hip alone; no byte outside a plane's [lo, hi) is read by anything here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {
// The contiguous RGB source is ImgArgs::img: its staging loop takes no source arguments.
struct NoSrc {};

// The NV12 source (Src::NV12, Src::NV21: a Y plane [B][h][w] and an interleaved UV plane [B][(h+1)/2][(w+1)/2][2]).
// [ylo, yhi) and [uvlo, uvhi) are the storage the planes live in: no byte outside them is read. tab: the colour
// matrix in 16.16 fixed point, row c = (Y, U, V) coefficients of channel c, then the offsets taken from Y, U and V
// first (ops/image.py builds it).
struct Nv12Args {
  const uint8_t *y, *uv;
  uintptr_t ylo, yhi, uvlo, uvhi;
  long long ypitch, uvpitch, ybs, uvbs;
  int tab[12];
};

// One plane of a source that is read through pitches: p its first byte, [lo, hi) the storage it lives in
// (no byte outside is read), pitch and bs the bytes between rows and between batch elements.
struct PlaneArg {
  const uint8_t* p;
  uintptr_t lo, hi;
  long long pitch, bs;
};

// Planar 4:2:0 (I420; YV12 is the same with u and v exchanged by the host): y [B][h][w], u and v
// [B][(h+1)/2][(w+1)/2]; tab as in Nv12Args.
struct PlanarArgs {
  PlaneArg y, u, v;
  int tab[12];
};

// Packed pixels [B][h][w][C], C = 3 or 4 by the instantiation: r, g, b are the byte offsets of red, green
// and blue inside a pixel (0, 1, 2 for RGB and RGBA; 2, 1, 0 for BGR and BGRA).
struct PackedArgs {
  PlaneArg s;
  int r, g, b;
};

// B tiles of one packed frame: tile b's first byte is s.p + origin[b] (a device table of byte offsets the host
// built from the tile origins) instead of s.p + b * s.bs.
struct PackedTileArgs : PackedArgs {
  const long long* origin;  // [B]
};

// The source of the general YUV front end: NosYuvSrc's runtime fields (all wave-uniform) and its planes; what
// the instantiation fixes (layout, hsub, sample bytes) is not repeated here. mask = 2^depth - 1.
struct YuvArgs {
  PlaneArg pl[3];
  int tab[12];
  int vsub, depth, shift, mask, order;
};
// What the bilinear instantiations (Yuv<..., 1>) take beside it: the chroma planes' columns and rows, and the
// weights in quarters of the two taps of an even and of an odd luma position, horizontally (wx) and vertically
// (wy), by the siting.
struct YuvBilinearArgs : YuvArgs {
  int cw, ch;
  int wx[4], wy[4];
};
// What the HDR instantiations (Hdr<Yuv<...>>) take beside that: the two tables of image_yuv.h's NosYuvHdr (device
// memory, the same for every thread: they live in L2 and the vector cache), lut1's entries and the gamut matrix by rows.
struct YuvHdrArgs : YuvBilinearArgs {
  const uint16_t* lut1;
  const uint8_t* lut2;
  int entries;
  int gamut[9];
};
// B tiles of one YUV frame (Src::YUV_TILES): tile b's first row and column are origin[2 * b] and origin[2 * b + 1], a
// device table a graph replays, so it is trusted for nothing: h and w are the frame's, and a patch whose footprint,
// shifted by the origin, does not lie inside them is skipped. The planes are one frame's (batch element 0).
struct TileFrame {
  const int* origin;  // [B][2]
  int h, w;
};
template <class A>
struct Tiled : A {
  TileFrame f;
};
template <class A>
constexpr bool IS_TILED = false;
template <class A>
constexpr bool IS_TILED<Tiled<A>> = true;

enum { YUV_PLANAR = 0, YUV_SEMI = 1, YUV_PACKED = 2 };
template <int LAYOUT_, int HSUB_, int SB_, int CHROMA_ = 0>
struct Yuv {
  static constexpr int LAYOUT = LAYOUT_, HSUB = HSUB_, SB = SB_, CHROMA = CHROMA_;
};
struct NoYuv {
  static constexpr int LAYOUT = -1, HSUB = 0, SB = 1, CHROMA = 0;
};
// a Yuv<...> whose codes are PQ or HLG: staged through the tables of YuvHdrArgs
template <class Y>
struct Hdr : Y {};
template <class Y>
constexpr bool IS_HDR = false;
template <class Y>
constexpr bool IS_HDR<Hdr<Y>> = true;

// four bytes at q, of which those inside [lo, hi) are read: one aligned dword where q allows it
__device__ __forceinline__ uint32_t load4(uintptr_t q, uintptr_t lo, uintptr_t hi) {
  if ((q & 3) == 0 && q >= lo && q + 4 <= hi) return *reinterpret_cast<const uint32_t*>(q);
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (q + k >= lo && q + k < hi) v |= uint32_t(*reinterpret_cast<const uint8_t*>(q + k)) << (8 * k);
  return v;
}

// NB bytes at any q into (NB + 3) / 4 dwords, lowest address first: load4 of the aligned dwords that hold
// them (one more than the result when q's alignment makes the bytes straddle it), shifted into place. Only
// bytes inside [lo, hi) are read; the others come out as zero.
template <int NB>
__device__ __forceinline__ void load_bytes(uint32_t* w, uintptr_t q, uintptr_t lo, uintptr_t hi) {
  constexpr int N = (NB + 3) / 4;
  const int sh = int(q & 3);
  const uintptr_t q0 = q - sh;
  uint32_t d[N + 1];
#pragma unroll
  for (int k = 0; k < N; ++k) d[k] = load4(q0 + 4 * k, lo, hi);
  d[N] = sh + NB > 4 * N ? load4(q0 + 4 * N, lo, hi) : 0u;
#pragma unroll
  for (int k = 0; k < N; ++k) w[k] = uint32_t((uint64_t(d[k + 1]) << 32 | d[k]) >> (8 * sh));
}

// four pixels (R | G << 8 | B << 16 each) as the 12 RGB bytes of a column group in the LDS tile
__device__ __forceinline__ void store_rgb4(uint32_t* dst, const uint32_t (&px)[4]) {
  dst[0] = px[0] | px[1] << 24;
  dst[1] = px[1] >> 8 | px[2] << 16;
  dst[2] = px[2] >> 16 | px[3] << 8;
}

// one pixel's channel c as 8.16 fixed point clamped to [0, 256): exact in int32 (the largest term is below
// 2^25, the sum below 2^27). The channel is bits 16-23, clip((sum + 2^15) >> 16, 0, 255) of ops/image.py:
// clamping before the shift is the same number. It is also deliberate: from clamp(x >> 16) | clamp(y >> 16)
// << 8 hipcc (ROCm 7) makes one v_ashr_pk_u8_i32 and takes that result's upper half for zero, which an
// MI355X does not deliver: the bytes OR-ed in above it came out wrong.
// The products are 24-bit multiplies (full rate; a 32-bit one is a quarter of it, and these 36 per thread
// were what the staging loop waited on): the host checks that every coefficient fits.
__device__ __forceinline__ uint32_t nv12_channel(const int* t, int c, int y, int u, int v) {
  return uint32_t(min(max(__mul24(t[3 * c], y) + __mul24(t[3 * c + 1], u) + __mul24(t[3 * c + 2], v) + 32768, 0),
                      0xffffff));
}

// Four columns of 4:2:0 as a column group of the LDS tile: yy their luma bytes, chroma(i, 0) and chroma(i, 1)
// the U and V sample under columns 2i and 2i + 1 (nearest: luma (r, c) takes chroma (r >> 1, c >> 1)).
template <class Chroma>
__device__ __forceinline__ void yuv_to_rgb4(const int* tab, uint32_t yy, Chroma chroma, uint32_t* dst) {
  uint32_t px[4];  // R | G << 8 | B << 16 of the group's four columns
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = int((yy >> (8 * k)) & 255) - tab[9];
    const int u = int(chroma(k >> 1, 0)) - tab[10];
    const int v = int(chroma(k >> 1, 1)) - tab[11];
    px[k] = nv12_channel(tab, 0, y, u, v) >> 16 | (nv12_channel(tab, 1, y, u, v) >> 8 & 0xff00) |
            (nv12_channel(tab, 2, y, u, v) & 0xff0000);
  }
  store_rgb4(dst, px);
}

// nv12_channel at any sample depth: the table is scaled by 2^(8 + depth), so the sum is clamped to
// [0, 2^(16 + depth)) and the channel is its bits from 8 + depth up (clamp, then shift: see nv12_channel).
// Exact in int32: the host checks the coefficients (24 bits) and the sum stays below 2^30 up to depth 12.
__device__ __forceinline__ uint32_t yuv_channel(const int* t, int c, int y, int u, int v, int depth) {
  const int s = __mul24(t[3 * c], y) + __mul24(t[3 * c + 1], u) + __mul24(t[3 * c + 2], v) + (1 << (7 + depth));
  return uint32_t(min(max(s, 0), (1 << (16 + depth)) - 1)) >> (8 + depth);
}

// One pixel of a PQ or HLG source as R | G << 8 | B << 16 (y, u, v: the codes less the table's offsets). The matrix's
// sums as in yuv_channel, but cut to codes k of the source's depth (the table is scaled by 2^(8 + depth): clamp to
// [0, 2^(16 + depth)) after adding 2^15, then shift by 16); l = lut1[k] is tone-mapped linear light, 16383 = SDR
// white; the gamut matrix in 2^-12 fixed point, clip((sum + 2048) >> 12, 0, 16383); lut2 of that is the sRGB byte.
// Exact in int32 with 24-bit multiplies: the host checks the gamut (below 2^15), l is below 2^14, the sums below 2^29.
// The indices cannot leave the tables: k < entries (the host checks entries == 2^depth) and the sum is clipped to
// lut2's 16384 entries.
__device__ __forceinline__ uint32_t hdr_pixel(const YuvHdrArgs& n, int y, int u, int v) {
  int l[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int s = __mul24(n.tab[3 * c], y) + __mul24(n.tab[3 * c + 1], u) + __mul24(n.tab[3 * c + 2], v) + 32768;
    const int k = int(uint32_t(min(max(s, 0), (1 << (16 + n.depth)) - 1)) >> 16);
    l[c] = n.lut1[min(k, n.entries - 1)];
  }
  uint32_t px = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int s = (__mul24(n.gamut[3 * c], l[0]) + __mul24(n.gamut[3 * c + 1], l[1]) +
                   __mul24(n.gamut[3 * c + 2], l[2]) + 2048) >> 12;
    px |= uint32_t(n.lut2[min(max(s, 0), 16383)]) << (8 * c);
  }
  return px;
}

// sample k of the dwords w (lowest address first): a byte, or a little-endian 16-bit word's code
template <int SB>
__device__ __forceinline__ int yuv_sample(const uint32_t* w, int k, int shift, int mask) {
  if constexpr (SB == 1) return int((w[k >> 2] >> (8 * (k & 3))) & 255u);
  else return int((((w[k >> 1] >> (16 * (k & 1))) & 0xffffu) >> shift) & uint32_t(mask));
}

// Four columns sx .. sx + 3 of row sy of a Yuv<layout, hsub, sample bytes> source as a column group of the LDS
// tile: planar, semi-planar or packed 4:2:2 (YUY2 / UYVY / YVYU); 4:2:0, 4:2:2 or 4:4:4; 8-bit samples, or 10 /
// 12-bit codes in 16-bit words (P010's high bits, yuv420p10le's low bits), by a table scaled to the depth.
// Nearest chroma: luma (r, c) takes chroma (r >> vsub, c >> hsub), so the group has 4 >> hsub chroma
// samples under it. Reads: 4 * SB luma bytes and (4 >> hsub) * SB bytes of each chroma plane (planar), or
// twice that of the interleaved pairs (semi-planar), or the group's two 4-byte macropixels in one read (packed).
// A: YuvArgs, or YuvHdrArgs of an Hdr<Yuv<...>>, whose pixels are hdr_pixel's instead (the same reads and chroma).
template <class Y, class A>
__device__ __forceinline__ void stage_yuv(const A& n, int b, int sy, int sx, uint32_t* dst) {
  constexpr int SB = Y::SB, HSUB = Y::HSUB, NC = 4 >> HSUB;
  const int depth = SB == 1 ? 8 : n.depth, shift = SB == 1 ? 0 : n.shift, mask = SB == 1 ? 255 : n.mask;
  int yy[4], uu[4], vv[4];
  if constexpr (Y::LAYOUT == YUV_PACKED) {
    // a macropixel is Y0 U Y1 V (0), U Y0 V Y1 (1) or Y0 V Y1 U (2): bit offsets of the first luma, U and V
    const PlaneArg& s = n.pl[0];
    const int ys = n.order == 1 ? 8 : 0, us = n.order == 0 ? 8 : n.order == 1 ? 0 : 24,
              vs = n.order == 0 ? 24 : n.order == 1 ? 16 : 8;
    uint32_t w[2];
    load_bytes<8>(w, reinterpret_cast<uintptr_t>(s.p) + b * s.bs + sy * s.pitch + sx * 2, s.lo, s.hi);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      yy[2 * i] = int((w[i] >> ys) & 255u), yy[2 * i + 1] = int((w[i] >> (16 + ys)) & 255u);
      uu[i] = int((w[i] >> us) & 255u), vv[i] = int((w[i] >> vs) & 255u);
    }
  } else {
    const PlaneArg& py = n.pl[0];
    uint32_t wy[SB];
    load_bytes<4 * SB>(wy, reinterpret_cast<uintptr_t>(py.p) + b * py.bs + sy * py.pitch + sx * SB, py.lo, py.hi);
#pragma unroll
    for (int k = 0; k < 4; ++k) yy[k] = yuv_sample<SB>(wy, k, shift, mask);
    const int cy = sy >> n.vsub, cx = sx >> HSUB;
    if constexpr (Y::LAYOUT == YUV_PLANAR) {
      const PlaneArg &pu = n.pl[1], &pv = n.pl[2];
      uint32_t wu[(NC * SB + 3) / 4], wv[(NC * SB + 3) / 4];
      load_bytes<NC * SB>(wu, reinterpret_cast<uintptr_t>(pu.p) + b * pu.bs + cy * pu.pitch + cx * SB, pu.lo, pu.hi);
      load_bytes<NC * SB>(wv, reinterpret_cast<uintptr_t>(pv.p) + b * pv.bs + cy * pv.pitch + cx * SB, pv.lo, pv.hi);
#pragma unroll
      for (int i = 0; i < NC; ++i) uu[i] = yuv_sample<SB>(wu, i, shift, mask), vv[i] = yuv_sample<SB>(wv, i, shift, mask);
    } else {
      // pairs of (U, V), or (V, U) with order 1
      const PlaneArg& pc = n.pl[1];
      uint32_t wc[(2 * NC * SB + 3) / 4];
      load_bytes<2 * NC * SB>(wc, reinterpret_cast<uintptr_t>(pc.p) + b * pc.bs + cy * pc.pitch + cx * 2 * SB, pc.lo,
                              pc.hi);
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const int c0 = yuv_sample<SB>(wc, 2 * i, shift, mask), c1 = yuv_sample<SB>(wc, 2 * i + 1, shift, mask);
        uu[i] = n.order ? c1 : c0, vv[i] = n.order ? c0 : c1;
      }
    }
  }
  uint32_t px[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = yy[k] - n.tab[9], u = uu[k >> HSUB] - n.tab[10], v = vv[k >> HSUB] - n.tab[11];
    if constexpr (IS_HDR<Y>)
      px[k] = hdr_pixel(n, y, u, v);
    else
      px[k] = yuv_channel(n.tab, 0, y, u, v, depth) | yuv_channel(n.tab, 1, y, u, v, depth) << 8 |
              yuv_channel(n.tab, 2, y, u, v, depth) << 16;
  }
  store_rgb4(dst, px);
}

// The chroma samples of columns 2g - 1 .. 2g + 2 of chroma row cy (inside the plane) of a Yuv<layout, 1, sample
// bytes> source: what the column group 4g needs of that row for bilinear chroma. One read per plane of the
// window's bytes inside [lo, hi), wherever they start (at g = 0 one sample before the row); then the columns are
// clamped by index to 0 .. cw - 1 (columns 2g and, with it, one clamped neighbour always lie inside the window),
// so whatever a read found outside the row — pitch padding, the neighbouring row, the other plane, zeros past the
// storage — is dropped here.
template <class Y>
__device__ __forceinline__ void chroma_window(const YuvBilinearArgs& n, int b, int sy, int cy, int g, int shift,
                                              int mask, int (&uu)[4], int (&vv)[4]) {
  constexpr int SB = Y::SB;
  if constexpr (Y::LAYOUT == YUV_PACKED) {
    // macropixels 2g - 1 .. 2g + 2 of the luma row: see stage_yuv for the orders
    const PlaneArg& s = n.pl[0];
    const int us = n.order == 0 ? 8 : n.order == 1 ? 0 : 24, vs = n.order == 0 ? 24 : n.order == 1 ? 16 : 8;
    uint32_t w[4];
    load_bytes<16>(w, reinterpret_cast<uintptr_t>(s.p) + b * s.bs + sy * s.pitch + (2 * g - 1) * 4, s.lo, s.hi);
#pragma unroll
    for (int k = 0; k < 4; ++k) uu[k] = int((w[k] >> us) & 255u), vv[k] = int((w[k] >> vs) & 255u);
  } else if constexpr (Y::LAYOUT == YUV_PLANAR) {
    const PlaneArg &pu = n.pl[1], &pv = n.pl[2];
    uint32_t wu[SB], wv[SB];
    load_bytes<4 * SB>(wu, reinterpret_cast<uintptr_t>(pu.p) + b * pu.bs + cy * pu.pitch + (2 * g - 1) * SB, pu.lo,
                       pu.hi);
    load_bytes<4 * SB>(wv, reinterpret_cast<uintptr_t>(pv.p) + b * pv.bs + cy * pv.pitch + (2 * g - 1) * SB, pv.lo,
                       pv.hi);
#pragma unroll
    for (int k = 0; k < 4; ++k) uu[k] = yuv_sample<SB>(wu, k, shift, mask), vv[k] = yuv_sample<SB>(wv, k, shift, mask);
  } else {
    const PlaneArg& pc = n.pl[1];
    uint32_t wc[2 * SB];
    load_bytes<8 * SB>(wc, reinterpret_cast<uintptr_t>(pc.p) + b * pc.bs + cy * pc.pitch + (2 * g - 1) * 2 * SB, pc.lo,
                       pc.hi);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c0 = yuv_sample<SB>(wc, 2 * k, shift, mask), c1 = yuv_sample<SB>(wc, 2 * k + 1, shift, mask);
      uu[k] = n.order ? c1 : c0, vv[k] = n.order ? c0 : c1;
    }
  }
  // window sample k is column 2g - 1 + k: inside the row for 1 - (g > 0) <= k <= cw - 2g (which is at least 1)
  const int kmax = n.cw - 2 * g;
  uu[0] = g ? uu[0] : uu[1], vv[0] = g ? vv[0] : vv[1];
  uu[2] = kmax >= 2 ? uu[2] : uu[1], vv[2] = kmax >= 2 ? vv[2] : vv[1];
  uu[3] = kmax >= 3 ? uu[3] : uu[2], vv[3] = kmax >= 3 ? vv[3] : vv[2];
}

// 4 x the horizontally upsampled samples under the group's four columns, from a row's window c: columns 4g and
// 4g + 2 take window samples (0, 1) and (1, 2) by the even weights wx[0..1], columns 4g + 1 and 4g + 3 take
// (1, 2) and (2, 3) by the odd weights wx[2..3]. 24-bit multiplies, as nv12_channel's.
__device__ __forceinline__ void chroma_row4(const int* wx, const int (&c)[4], int (&h)[4]) {
  h[0] = __mul24(wx[0], c[0]) + __mul24(wx[1], c[1]);
  h[1] = __mul24(wx[2], c[1]) + __mul24(wx[3], c[2]);
  h[2] = __mul24(wx[0], c[1]) + __mul24(wx[1], c[2]);
  h[3] = __mul24(wx[2], c[2]) + __mul24(wx[3], c[3]);
}

// stage_yuv with bilinear chroma (hsub = 1): luma position x has i = x >> 1 and takes two chroma samples with
// weights in quarters — co-sited (4, 0) of C[i], C[i] at an even x and (2, 2) of C[i], C[i + 1] at an odd one,
// centred (1, 3) of C[i - 1], C[i] and (3, 1) of C[i], C[i + 1] — on each subsampled axis, indices clamped to the
// plane; the sample is (sum of wy wx C + 8) >> 4, a code of the source's depth that goes through the table as
// the nearest one does. n.wx / n.wy hold (w of the lower tap, w of the upper) for even, then for odd positions;
// the lower tap of an even position is C[i - 1] (weight 0 when co-sited). Reads: the luma as stage_yuv, and the
// chroma window (chroma_window) of one row (4:2:2) or two (4:2:0): each thread reads its group's window straight
// from the planes (no chroma tile in LDS).
// A: YuvBilinearArgs, or YuvHdrArgs as in stage_yuv.
template <class Y, class A>
__device__ __forceinline__ void stage_yuv_bilinear(const A& n, int b, int sy, int sx, uint32_t* dst) {
  constexpr int SB = Y::SB;
  static_assert(Y::HSUB == 1, "bilinear chroma is for horizontally subsampled sources");
  const int depth = SB == 1 ? 8 : n.depth, shift = SB == 1 ? 0 : n.shift, mask = SB == 1 ? 255 : n.mask;
  const int g = sx >> 2;
  int yy[4];
  if constexpr (Y::LAYOUT == YUV_PACKED) {
    const PlaneArg& s = n.pl[0];
    const int ys = n.order == 1 ? 8 : 0;
    uint32_t w[2];
    load_bytes<8>(w, reinterpret_cast<uintptr_t>(s.p) + b * s.bs + sy * s.pitch + sx * 2, s.lo, s.hi);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      yy[2 * i] = int((w[i] >> ys) & 255u), yy[2 * i + 1] = int((w[i] >> (16 + ys)) & 255u);
  } else {
    const PlaneArg& py = n.pl[0];
    uint32_t wy[SB];
    load_bytes<4 * SB>(wy, reinterpret_cast<uintptr_t>(py.p) + b * py.bs + sy * py.pitch + sx * SB, py.lo, py.hi);
#pragma unroll
    for (int k = 0; k < 4; ++k) yy[k] = yuv_sample<SB>(wy, k, shift, mask);
  }
  int su[4], sv[4];  // 16 x the upsampled samples
  int cu[4], cv[4], hu[4], hv[4];
  if (n.vsub) {
    // vertically: an even row takes chroma rows (cy - 1, cy), an odd one (cy, cy + 1), clamped by index
    const int odd = sy & 1, r0 = (sy >> 1) - 1 + odd;
    const int w0 = odd ? n.wy[2] : n.wy[0], w1 = odd ? n.wy[3] : n.wy[1];
    chroma_window<Y>(n, b, sy, min(max(r0, 0), n.ch - 1), g, shift, mask, cu, cv);
    chroma_row4(n.wx, cu, hu), chroma_row4(n.wx, cv, hv);
#pragma unroll
    for (int k = 0; k < 4; ++k) su[k] = __mul24(w0, hu[k]), sv[k] = __mul24(w0, hv[k]);
    chroma_window<Y>(n, b, sy, min(r0 + 1, n.ch - 1), g, shift, mask, cu, cv);
    chroma_row4(n.wx, cu, hu), chroma_row4(n.wx, cv, hv);
#pragma unroll
    for (int k = 0; k < 4; ++k) su[k] += __mul24(w1, hu[k]), sv[k] += __mul24(w1, hv[k]);
  } else {
    chroma_window<Y>(n, b, sy, sy, g, shift, mask, cu, cv);
    chroma_row4(n.wx, cu, hu), chroma_row4(n.wx, cv, hv);
#pragma unroll
    for (int k = 0; k < 4; ++k) su[k] = hu[k] << 2, sv[k] = hv[k] << 2;
  }
  uint32_t px[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = yy[k] - n.tab[9], u = ((su[k] + 8) >> 4) - n.tab[10], v = ((sv[k] + 8) >> 4) - n.tab[11];
    if constexpr (IS_HDR<Y>)
      px[k] = hdr_pixel(n, y, u, v);
    else
      px[k] = yuv_channel(n.tab, 0, y, u, v, depth) | yuv_channel(n.tab, 1, y, u, v, depth) << 8 |
              yuv_channel(n.tab, 2, y, u, v, depth) << 16;
  }
  store_rgb4(dst, px);
}
}  // namespace

