// The image half of the workload (YOLOS-small): the pixels in front of the model and the detections
// behind it, each as one launch with no host synchronisation.
//
//  * image_patch_planes_u8 — a uint8 RGB image [B][h][w][3] straight to the patch-embedding GEMM's
//    operand: separable antialiased triangle resample to H x W (tap tables built on the host in fp64
//    and read as constants), the per-channel affine v * a_c + b_c, and the exact x3 split into the
//    three bf16 planes [3][B*gh*gw][3*p*p] of the patch matrix (row (b, i, j), column (c, u, v), as
//    patch_planes_f32 in head.hip); optionally the fp32 pixels [B][3][H][W] as well. One 256-thread
//    workgroup per p x p patch: the patch's source footprint is staged in LDS with aligned 4-byte
//    loads, resampled horizontally into an fp32 LDS tile, then vertically by thread (u, v).
//  * image_patch_planes_nv12 — the same kernel body with another staging loop: the source is a video
//    decoder's NV12 surface (a Y plane [B][h][w] and an interleaved UV plane [B][(h+1)/2][(w+1)/2][2],
//    each with its own row pitch and batch stride). The footprint's luma rows and the chroma rows under
//    them are read, converted to RGB by an integer matrix the host passes (nearest chroma: luma (r, c)
//    takes chroma (r >> 1, c >> 1)) and written as RGB bytes into the same LDS tile; everything behind
//    the staging loop is shared, so the result is bit-equal to the RGB kernel on the converted frame.
//  * image_patch_planes_nv21 / _yuv420p / _packed3 / _packed4 — further staging loops of that body, one
//    instantiation each (Src below): NV12 with V before U; planar 4:2:0 (I420 / YV12: three planes, each
//    with its own pitch, batch stride and storage); and packed pixels of 3 or 4 bytes (RGB, BGR, RGBA,
//    BGRA: the colour bytes at offsets the host passes, a fourth byte never read as colour) at any row
//    pitch, batch stride and alignment, so a crop or a padded capture buffer is read in place. All of them
//    write RGB bytes in column groups of 4 into the LDS tile, and share every pass behind it.
//  * image_patch_planes_yuv<Yuv<layout, hsub, sample bytes>> — the general YUV front end behind one descriptor
//    (image_yuv.h): planar, semi-planar or packed 4:2:2 (YUY2 / UYVY / YVYU); 4:2:0, 4:2:2 or 4:4:4; 8-bit
//    samples, or 10 / 12-bit codes in 16-bit words (P010's high bits, yuv420p10le's low bits), by a table scaled
//    to the depth. Again only a staging loop (stage_yuv); the six entries above are as they were.
//  * image_patch_planes_yuv_bilinear<Yuv<layout, 1, sample bytes, 1>> — the same with bilinear chroma at a siting
//    (stage_yuv_bilinear): five more instantiations, the subsampled layouts; each thread reads its group's chroma
//    window straight from the planes (no chroma tile in LDS).
//  * image_patch_planes_yuv_hdr<Yuv<layout, hsub, 2[, 1]>> — 10 / 12-bit sources whose codes are PQ or HLG, tone-mapped
//    to SDR: the two staging loops again, with hdr_pixel in place of yuv_channel — the R'G'B' codes at the source's
//    depth through a table, a 3 x 3 integer matrix and a second table (image_yuv.h's NosYuvHdr; the host builds them in
//    fp64 and the kernel knows no transfer function). Six more instantiations: planar and semi-planar, 4:4:4 and
//    subsampled with nearest chroma, subsampled with bilinear chroma.
//  * image_patch_planes_tiles3 / _tiles4 — the packed staging loops over B tiles of one frame: tile b starts at a byte
//    offset read from a device table (tile origins on a 2-D grid are not one batch stride); [lo, hi) stays the frame's
//    storage. Bit-equal to the packed entries on the B crops stacked.
//  * image_patch_planes_yuv_tiles / _yuv_bilinear_tiles / _yuv_hdr_tiles<Yuv<...>> — the three YUV front ends over B
//    tiles of one frame, the same instantiations: tile b's (first row, first column) is read from a device table (the
//    one merge_detections_f32 reads) and moves the patch's footprint into the frame before the column groups are laid
//    out, so the staging loops run unchanged on frame coordinates. Bit-equal to the tiles3 entry on the converted frame.
//  * detections_f32 — softmax over the class logits, the best of the first L classes, the box in
//    corner format scaled to the original image, and a stable compaction of the rows above the
//    threshold; one workgroup per image, one wave per row.
//  * merge_detections_f32 — the detections of B overlapping tiles of one frame as one list: scores as above, boxes in
//    frame pixels, the candidates ordered by score (a rank count in LDS), duplicates of another tile's kept box
//    suppressed greedily (one pivot per barrier), the kept rows compacted in that order; one workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "image_yuv.h"

namespace {
thread_local std::string g_err;

// TAPS: weights per output row / column (scale <= 4: 2 * 4 + 1); PMAX: patch side; FMAX: rows and
// columns of a patch's source footprint, at most scale * (p + 1) + 1 = 69 at scale 4 and p = 16
// (the host passes the largest footprint of the tables and it is checked against FMAX).
constexpr int TAPS = 9, PMAX = 16, FMAX = 72;
// a footprint row in LDS: the global row's bytes at its own alignment (0-3 bytes of lead-in), whole dwords
constexpr int NDW = (FMAX * 3 + 3 + 3) / 4, RS = NDW * 4;
constexpr int MMAX = 1024, CMAX = 128;
// the detections workgroup: 16 waves, so the 100 rows of YOLOS are 7 dependent row passes, not 25
constexpr int DT = 1024, DW = DT / 64;

struct ImgArgs {
  const uint8_t* img;   // [B][h][w][3]
  __bf16* planes;       // [3][B*gh*gw][3*p*p]
  float* pixels;        // [B][3][H][W] or null
  const int* yidx;      // [2][H]: first source row, tap count
  const float* ywt;     // [H][TAPS]
  const int* xidx;      // [2][W]
  const float* xwt;     // [W][TAPS]
  float a[3], b[3];
  int B, h, w, H, W, p, gh, gw, GH, GW;  // GH x GW: the tiles that cover H x W (>= gh x gw)
};

// The NV12 source of image_patch_planes_nv12. [ylo, yhi) and [uvlo, uvhi) are the storage the planes
// live in: no byte outside them is read. tab: the colour matrix in 16.16 fixed point, row c = (Y, U, V)
// coefficients of channel c, then the offsets taken from Y, U and V first (ops/image.py builds it).
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
// built from the tile origins) instead of s.p + b * s.bs. A type of its own, so that the packed kernels' arguments
// are what they were.
struct PackedTileArgs : PackedArgs {
  const long long* origin;  // [B]
};

// The source layouts, one instantiation of the body (and one __global__ entry) each. RGB: contiguous
// [B][h][w][3], staged as whole rows of aligned dwords, footprints of up to FMAX = 72 columns. Every other
// layout stages columns in groups of 4 (for 4:2:0 one dword of luma and the two chroma samples under it, for
// packed pixels 12 or 16 source bytes; three dwords of RGB out): NG groups fit a row of the LDS tile, and
// any GROUP_FMAX_W = 69 columns lie inside 18 consecutive groups wherever they start, so these layouts
// cover footprints of up to 69 columns (scale 4 at patch 16); the host falls back past that.
// YUV is the general front end (image_yuv.h): its staging loop is instantiated per Yuv<layout, hsub, sample bytes>.
enum class Src { RGB, NV12, NV21, YUV420P, PACKED3, PACKED4, YUV, TILES3, TILES4, YUV_TILES };
constexpr int NG = RS / 12, GROUP_FMAX_W = NG * 4 - 3;
constexpr int NV12_FMAX_W = GROUP_FMAX_W, YUV420P_FMAX_W = GROUP_FMAX_W, PACKED_FMAX_W = GROUP_FMAX_W;
constexpr int YUV_FMAX_W = GROUP_FMAX_W;

// The source of image_patch_planes_yuv_*: NosYuvSrc's runtime fields (all wave-uniform) and its planes; what
// the instantiation fixes (layout, hsub, sample bytes) is not repeated here. mask = 2^depth - 1.
struct YuvArgs {
  PlaneArg pl[3];
  int tab[12];
  int vsub, depth, shift, mask, order;
};
// What the bilinear instantiations (Yuv<..., 1>) take beside it: the chroma planes' columns and rows, and the
// weights in quarters of the two taps of an even and of an odd luma position, horizontally (wx) and vertically
// (wy), by the siting. A type of its own, so that the nearest kernels' arguments are what they were.
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
// shifted by the origin, does not lie inside them is skipped. The planes are one frame's (batch element 0). Types of
// their own, so that the untiled kernels' arguments are what they were.
struct TileFrame {
  const int* origin;  // [B][2]
  int h, w;
};
struct YuvTileArgs : YuvArgs {
  TileFrame f;
};
struct YuvBilinearTileArgs : YuvBilinearArgs {
  TileFrame f;
};
struct YuvHdrTileArgs : YuvHdrArgs {
  TileFrame f;
};
enum { YUV_PLANAR = 0, YUV_SEMI = 1, YUV_PACKED = 2 };
template <int LAYOUT_, int HSUB_, int SB_, int CHROMA_ = 0>
struct Yuv {
  static constexpr int LAYOUT = LAYOUT_, HSUB = HSUB_, SB = SB_, CHROMA = CHROMA_;
};
struct NoYuv {
  static constexpr int LAYOUT = -1, HSUB = 0, SB = 1, CHROMA = 0;
};
// a Yuv<...> whose codes are PQ or HLG: staged through the tables of YuvHdrArgs (a wrapper, so that the names of the
// older instantiations are what they were)
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
// tile. Nearest chroma: luma (r, c) takes chroma (r >> vsub, c >> hsub), so the group has 4 >> hsub chroma
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
// chroma window (chroma_window) of one row (4:2:2) or two (4:2:0).
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

// SrcArgs: what the layout's staging loop reads besides ImgArgs (Nv12Args, PlanarArgs, PackedArgs, YuvArgs,
// YuvBilinearArgs or YuvHdrArgs, or their ...TileArgs; the contiguous RGB source is ImgArgs::img and takes an empty
// Nv12Args). Y: Src::YUV's and Src::YUV_TILES' Yuv<...>.
// Src::YUV_TILES: ImgArgs' h x w is the tile, the tap tables are the tile's, and the footprint they give is moved by
// the tile's origin into the frame before the column groups are laid out: the groups are the frame's (whatever the
// parity of the origin, a chroma pair lies under its luma as in the untiled launch), and the staging loops run on
// frame coordinates with batch element 0, so bilinear chroma clamps at the frame's edge, not at the tile's.
template <Src S, class SrcArgs, class Y = NoYuv>
__device__ __forceinline__ void image_patch_planes_body(const ImgArgs& a, const SrcArgs& n) {
  constexpr bool GROUPS = S != Src::RGB;
  __shared__ __attribute__((aligned(16))) uint8_t src[FMAX * RS];
  __shared__ float hz[FMAX * PMAX * 3];  // [footprint row][v][c]: the horizontally resampled rows
  __shared__ float wxs[PMAX * TAPS], wys[PMAX * TAPS];
  __shared__ int xf[PMAX], xc[PMAX], yf[PMAX], yc[PMAX];
  const int tid = threadIdx.x, p = a.p, H = a.H, W = a.W;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(a.img), hi = lo + size_t(a.B) * a.h * a.w * 3;
  const int tiles = a.B * a.GH * a.GW;
  const size_t ck = size_t(3) * p * p, plane = size_t(a.B) * a.gh * a.gw * ck;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int b = t / (a.GH * a.GW), ij = t % (a.GH * a.GW), i = ij / a.GW, j = ij % a.GW;
    const int y0 = i * p, x0 = j * p, ny = min(p, H - y0), nx = min(p, W - x0);
    // the footprint: first source row / column of the first output, one past the last of the last
    // (both ends grow with the output index)
    const int fy0 = a.yidx[y0], fy1 = a.yidx[y0 + ny - 1] + a.yidx[H + y0 + ny - 1];
    const int fx0 = a.xidx[x0], fx1 = a.xidx[x0 + nx - 1] + a.xidx[W + x0 + nx - 1];
    const int fh = fy1 - fy0, fw = fx1 - fx0;
    // the host checked the tables against these limits; a table that breaks them reads nothing
    if (fy0 < 0 || fx0 < 0 || fy1 > a.h || fx1 > a.w || fh <= 0 || fw <= 0 || fh > FMAX || fw > FMAX) continue;
    // tiles of a YUV frame: the tile's origin, read once per patch (b is the block's, so every lane reads the same
    // pair; readfirstlane says so to the compiler, which keeps what follows from it in scalar registers); a footprint
    // that it does not leave inside the frame reads nothing (fy1 and fx1 are positive: no overflow)
    int oy = 0, ox = 0;
    if constexpr (S == Src::YUV_TILES) {
      oy = __builtin_amdgcn_readfirstlane(n.f.origin[2 * b]);
      ox = __builtin_amdgcn_readfirstlane(n.f.origin[2 * b + 1]);
      if (oy < 0 || ox < 0 || oy > n.f.h - fy1 || ox > n.f.w - fx1) continue;
    }
    // all but RGB: column groups of 4, the first one holding fx0; lead bytes of a row in LDS, groups per row
    const int sx0 = fx0 + ox, sx1 = fx1 + ox, sy0 = fy0 + oy;  // the footprint in the source's coordinates
    const int gx0 = sx0 >> 2, lead = (sx0 & 3) * 3, ng = ((sx1 - 1) >> 2) - gx0 + 1;
    if (GROUPS && ng > NG) continue;
    __syncthreads();  // the previous tile's readers are done with the LDS
    if (tid < ny * TAPS) wys[tid] = a.ywt[size_t(y0) * TAPS + tid];
    if (tid < nx * TAPS) wxs[tid] = a.xwt[size_t(x0) * TAPS + tid];
    if (tid < ny) {
      yf[tid] = min(max(a.yidx[y0 + tid] - fy0, 0), fh - 1);
      yc[tid] = min(min(a.yidx[H + y0 + tid], TAPS), fh - yf[tid]);
    }
    if (tid < nx) {
      xf[tid] = min(max(a.xidx[x0 + tid] - fx0, 0), fw - 1);
      xc[tid] = min(min(a.xidx[W + x0 + tid], TAPS), fw - xf[tid]);
    }
    if constexpr (GROUPS) {
      // stage the footprint as RGB bytes: thread (row r, group g) reads the group's four columns, makes RGB
      // of them and writes 12 bytes (columns outside the footprint, at the two ends of a row, get bytes no
      // later pass reads; pitch padding, a neighbouring row's or another plane's bytes can only land there)
      for (int e = tid; e < fh * NG; e += 256) {
        const int r = e / NG, g = e % NG;
        if (g >= ng) continue;
        const int sy = sy0 + r, sx = (gx0 + g) * 4;
        uint32_t* dst = reinterpret_cast<uint32_t*>(src + r * RS + g * 12);
        if constexpr (S == Src::NV12 || S == Src::NV21) {
          // 4 luma bytes and the 2 chroma pairs under them; NV21 has V in a pair's first byte
          constexpr int UB = S == Src::NV21 ? 8 : 0;
          const uintptr_t qy = reinterpret_cast<uintptr_t>(n.y) + b * n.ybs + sy * n.ypitch + sx;
          const uintptr_t qc = reinterpret_cast<uintptr_t>(n.uv) + b * n.uvbs + (sy >> 1) * n.uvpitch + sx;
          const uint32_t yy = load4(qy, n.ylo, n.yhi), cc = load4(qc, n.uvlo, n.uvhi);
          yuv_to_rgb4(n.tab, yy, [cc](int i, int v) { return (cc >> (16 * i + (v ? 8 - UB : UB))) & 255; }, dst);
        } else if constexpr (S == Src::YUV420P) {
          // 4 luma bytes, and 2 bytes of each chroma plane: every plane by its own pitch and batch stride
          const uintptr_t qy = reinterpret_cast<uintptr_t>(n.y.p) + b * n.y.bs + sy * n.y.pitch + sx;
          const uintptr_t qu = reinterpret_cast<uintptr_t>(n.u.p) + b * n.u.bs + (sy >> 1) * n.u.pitch + (sx >> 1);
          const uintptr_t qv = reinterpret_cast<uintptr_t>(n.v.p) + b * n.v.bs + (sy >> 1) * n.v.pitch + (sx >> 1);
          uint32_t uu, vv;
          load_bytes<2>(&uu, qu, n.u.lo, n.u.hi);
          load_bytes<2>(&vv, qv, n.v.lo, n.v.hi);
          yuv_to_rgb4(n.tab, load4(qy, n.y.lo, n.y.hi),
                      [uu, vv](int i, int v) { return ((v ? vv : uu) >> (8 * i)) & 255; }, dst);
        } else if constexpr (S == Src::YUV) {
          if constexpr (Y::CHROMA == 1) stage_yuv_bilinear<Y>(n, b, sy, sx, dst);
          else stage_yuv<Y>(n, b, sy, sx, dst);
        } else if constexpr (S == Src::YUV_TILES) {
          if constexpr (Y::CHROMA == 1) stage_yuv_bilinear<Y>(n, 0, sy, sx, dst);
          else stage_yuv<Y>(n, 0, sy, sx, dst);
        } else {
          // 4 pixels of C = 3 or 4 bytes: their 12 or 16 bytes from the row's aligned dwords, then the three
          // colour bytes of each by their offsets in a pixel (a fourth byte is dropped here)
          constexpr int C = S == Src::PACKED4 || S == Src::TILES4 ? 4 : 3;
          uint32_t w[C], px[4];
          long long first;  // of image b: by the batch stride, or (tiles of one frame) from the origin table
          if constexpr (S == Src::TILES3 || S == Src::TILES4) first = n.origin[b];
          else first = b * n.s.bs;
          load_bytes<4 * C>(w, reinterpret_cast<uintptr_t>(n.s.p) + first + sy * n.s.pitch + sx * C, n.s.lo, n.s.hi);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            uint32_t q;  // pixel k's bytes from bit 0
            if constexpr (C == 4) q = w[k];
            else q = k == 0 ? w[0] : k == 1 ? (w[0] >> 24 | w[1] << 8) : k == 2 ? (w[1] >> 16 | w[2] << 16) : w[2] >> 8;
            px[k] = (q >> (8 * n.r) & 255) | (q >> (8 * n.g) & 255) << 8 | (q >> (8 * n.b) & 255) << 16;
          }
          store_rgb4(dst, px);
        }
      }
    } else {
      // stage the footprint: aligned dwords of each global row (the row's own alignment kept in LDS)
      const int rowbytes = fw * 3;
      for (int e = tid; e < fh * NDW; e += 256) {
        const int r = e / NDW, d = e % NDW;
        const uintptr_t addr = lo + ((size_t(b) * a.h + fy0 + r) * a.w + fx0) * 3;
        const int sh = int(addr & 3);
        if (d * 4 >= sh + rowbytes) continue;
        const uintptr_t q = addr - sh + size_t(d) * 4;
        uint32_t v = 0;
        if (q >= lo && q + 4 <= hi) {
          v = *reinterpret_cast<const uint32_t*>(q);
        } else {  // the dword that straddles an end of the image: its bytes inside, one by one
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (q + k >= lo && q + k < hi) v |= uint32_t(*reinterpret_cast<const uint8_t*>(q + k)) << (8 * k);
        }
        *reinterpret_cast<uint32_t*>(src + r * RS + d * 4) = v;
      }
    }
    __syncthreads();
    // horizontal pass: (footprint row r, output column v, channel c), taps in ascending order
    for (int e = tid; e < fh * PMAX * 3; e += 256) {
      const int c = e % 3, v = (e / 3) % PMAX, r = e / (3 * PMAX);
      if (v >= nx) continue;
      int sh = lead;
      if constexpr (!GROUPS) sh = int((lo + ((size_t(b) * a.h + fy0 + r) * a.w + fx0) * 3) & 3);
      const uint8_t* s = src + r * RS + sh + xf[v] * 3 + c;
      const float* wt = wxs + v * TAPS;
      float acc = 0.f;
      for (int k = 0; k < xc[v]; ++k) acc = fmaf(wt[k], float(s[k * 3]), acc);
      hz[e] = acc;
    }
    __syncthreads();
    // vertical pass, affine, split and store: thread (u, v), three channels
    const bool in_grid = i < a.gh && j < a.gw;
    const size_t row = (size_t(b) * a.gh + i) * a.gw + j;
    for (int e = tid; e < p * p; e += 256) {
      const int u = e / p, v = e % p;
      if (u >= ny || v >= nx) continue;
      const float* wt = wys + u * TAPS;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* hcol = hz + (yf[u] * PMAX + v) * 3 + c;
        float acc = 0.f;
        for (int k = 0; k < yc[u]; ++k) acc = fmaf(wt[k], hcol[k * PMAX * 3], acc);
        const float val = fmaf(acc, a.a[c], a.b[c]);
        if (a.pixels != nullptr) a.pixels[((size_t(b) * 3 + c) * H + y0 + u) * W + x0 + v] = val;
        if (in_grid) {
          const __bf16 h0 = (__bf16)val;
          const float r1 = val - (float)h0;
          const __bf16 h1 = (__bf16)r1;
          const __bf16 h2 = (__bf16)(r1 - (float)h1);
          const size_t o = row * ck + size_t(c) * p * p + e;
          a.planes[o] = h0;
          a.planes[plane + o] = h1;
          a.planes[2 * plane + o] = h2;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void image_patch_planes_u8(ImgArgs a) {
  image_patch_planes_body<Src::RGB>(a, Nv12Args{});
}

__global__ __launch_bounds__(256) void image_patch_planes_nv12(ImgArgs a, Nv12Args n) {
  image_patch_planes_body<Src::NV12>(a, n);
}

__global__ __launch_bounds__(256) void image_patch_planes_nv21(ImgArgs a, Nv12Args n) {
  image_patch_planes_body<Src::NV21>(a, n);
}

__global__ __launch_bounds__(256) void image_patch_planes_yuv420p(ImgArgs a, PlanarArgs n) {
  image_patch_planes_body<Src::YUV420P>(a, n);
}

__global__ __launch_bounds__(256) void image_patch_planes_packed3(ImgArgs a, PackedArgs n) {
  image_patch_planes_body<Src::PACKED3>(a, n);
}

__global__ __launch_bounds__(256) void image_patch_planes_packed4(ImgArgs a, PackedArgs n) {
  image_patch_planes_body<Src::PACKED4>(a, n);
}

__global__ __launch_bounds__(256) void image_patch_planes_tiles3(ImgArgs a, PackedTileArgs n) {
  image_patch_planes_body<Src::TILES3>(a, n);
}

__global__ __launch_bounds__(256) void image_patch_planes_tiles4(ImgArgs a, PackedTileArgs n) {
  image_patch_planes_body<Src::TILES4>(a, n);
}

// the general YUV front end: one instantiation per (layout, hsub, sample bytes) the host launches
template <class Y>
__global__ __launch_bounds__(256) void image_patch_planes_yuv(ImgArgs a, YuvArgs n) {
  image_patch_planes_body<Src::YUV, YuvArgs, Y>(a, n);
}

// the same with bilinear chroma: one instantiation per subsampled (layout, sample bytes)
template <class Y>
__global__ __launch_bounds__(256) void image_patch_planes_yuv_bilinear(ImgArgs a, YuvBilinearArgs n) {
  image_patch_planes_body<Src::YUV, YuvBilinearArgs, Y>(a, n);
}

// PQ and HLG sources, through the tables: one instantiation per (layout, hsub) of 16-bit samples with nearest chroma,
// and per layout with bilinear chroma (hsub = 1)
template <class Y>
__global__ __launch_bounds__(256) void image_patch_planes_yuv_hdr(ImgArgs a, YuvHdrArgs n) {
  image_patch_planes_body<Src::YUV, YuvHdrArgs, Hdr<Y>>(a, n);
}

// B tiles of one frame through the same three front ends: the same instantiations, the tile's origin from a table
template <class Y>
__global__ __launch_bounds__(256) void image_patch_planes_yuv_tiles(ImgArgs a, YuvTileArgs n) {
  image_patch_planes_body<Src::YUV_TILES, YuvTileArgs, Y>(a, n);
}

template <class Y>
__global__ __launch_bounds__(256) void image_patch_planes_yuv_bilinear_tiles(ImgArgs a, YuvBilinearTileArgs n) {
  image_patch_planes_body<Src::YUV_TILES, YuvBilinearTileArgs, Y>(a, n);
}

template <class Y>
__global__ __launch_bounds__(256) void image_patch_planes_yuv_hdr_tiles(ImgArgs a, YuvHdrTileArgs n) {
  image_patch_planes_body<Src::YUV_TILES, YuvHdrTileArgs, Hdr<Y>>(a, n);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// logits [B][M][C] (C = L + 1, the last class "no object"), boxes [B][M][4] (cx, cy, w, h in 0..1),
// target [B][2] (height, width) -> the rows with score > thr, in row order, at the front of
// scores / labels / out_boxes [B][M](x4), zeros behind them, and their number in count [B]
__global__ __launch_bounds__(DT) void detections_f32(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                      const float* __restrict__ target, float thr, int M, int C,
                                                      float* __restrict__ scores, int* __restrict__ labels,
                                                      float* __restrict__ out_boxes, int* __restrict__ count) {
  __shared__ float s_score[MMAX];
  __shared__ int s_label[MMAX];
  __shared__ int s_wave[DW];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, L = C - 1;
  for (int row = wave; row < M; row += DW) {
    const float* x = logits + (size_t(b) * M + row) * C;
    const float x0 = lane < C ? x[lane] : -INFINITY, x1 = lane + 64 < C ? x[lane + 64] : -INFINITY;
    const float m = wave_max(fmaxf(x0, x1));
    const float e0 = lane < C ? expf(x0 - m) : 0.f, e1 = lane + 64 < C ? expf(x1 - m) : 0.f;
    const float sum = wave_sum(e0 + e1);
    // the largest probability of the first L classes, the lowest index on ties
    float best = lane < L ? e0 / sum : -1.f;
    int idx = lane;
    const float p1 = lane + 64 < L ? e1 / sum : -1.f;
    if (p1 > best) best = p1, idx = lane + 64;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(idx, o);
      if (ob > best || (ob == best && oi < idx)) best = ob, idx = oi;
    }
    if (lane == 0) {
      s_score[row] = best;
      s_label[row] = idx;
    }
  }
  __syncthreads();
  const float th = target[2 * b], tw = target[2 * b + 1];
  int base = 0;  // kept rows so far: the same in every thread
  for (int r0 = 0; r0 < M; r0 += DT) {
    const int row = r0 + tid;
    const bool keep = row < M && s_score[row] > thr;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    int off = base;
    for (int k = 0; k < wave; ++k) off += s_wave[k];
    if (keep) {
      const size_t slot = size_t(b) * M + off + __popcll(mask & ((1ull << lane) - 1ull));
      const float* bx = boxes + (size_t(b) * M + row) * 4;
      const float cx = bx[0], cy = bx[1], hw = 0.5f * bx[2], hh = 0.5f * bx[3];
      scores[slot] = s_score[row];
      labels[slot] = s_label[row];
      out_boxes[slot * 4 + 0] = (cx - hw) * tw;
      out_boxes[slot * 4 + 1] = (cy - hh) * th;
      out_boxes[slot * 4 + 2] = (cx + hw) * tw;
      out_boxes[slot * 4 + 3] = (cy + hh) * th;
    }
    for (int k = 0; k < DW; ++k) base += s_wave[k];
    __syncthreads();  // s_wave is rewritten by the next chunk
  }
  for (int k = base + tid; k < M; k += DT) {
    const size_t slot = size_t(b) * M + k;
    scores[slot] = 0.f;
    labels[slot] = 0;
    out_boxes[slot * 4 + 0] = 0.f;
    out_boxes[slot * 4 + 1] = 0.f;
    out_boxes[slot * 4 + 2] = 0.f;
    out_boxes[slot * 4 + 3] = 0.f;
  }
  if (tid == 0) count[b] = base;
}

// overlap of two corner boxes: inter / min(area) (iou = 0, "intersection over smaller") or inter / union (iou = 1);
// a denominator that is not positive counts as overlap 0
__device__ __forceinline__ float box_overlap(const float* a, const float* b, int iou) {
  const float iw = fmaxf(fminf(a[2], b[2]) - fmaxf(a[0], b[0]), 0.f);
  const float ih = fmaxf(fminf(a[3], b[3]) - fmaxf(a[1], b[1]), 0.f);
  const float inter = iw * ih;
  const float aa = (a[2] - a[0]) * (a[3] - a[1]), ab = (b[2] - b[0]) * (b[3] - b[1]);
  const float den = iou ? aa + ab - inter : fminf(aa, ab);
  return den > 0.f ? inter / den : 0.f;
}

// logits [B][M][C] and boxes [B][M][4] of B tiles of th x tw pixels whose first pixel is origins[b] = (y0, x0) of one
// frame -> the rows with score > thr as one list in frame pixels, ordered by score descending (ties: row b * M + m
// ascending), less every row that an earlier kept row of the same label from another tile overlaps by more than mt;
// the kept rows at the front of scores / labels / out_boxes / tile [B*M], zeros behind them, their number in count[0].
// One workgroup, N = B * M <= MMAX. Static LDS: 10 tables of MMAX words = 40 KB.
__global__ __launch_bounds__(DT) void merge_detections_f32(const float* __restrict__ logits,
                                                            const float* __restrict__ boxes,
                                                            const int* __restrict__ origins, float th, float tw,
                                                            float thr, float mt, int iou, int N, int M, int C,
                                                            float* __restrict__ scores, int* __restrict__ labels,
                                                            float* __restrict__ out_boxes, int* __restrict__ tile,
                                                            int* __restrict__ count) {
  __shared__ float s_score[MMAX];   // by row
  __shared__ int s_label[MMAX];
  __shared__ float q_score[MMAX];   // by rank among the candidates
  __shared__ int q_label[MMAX], q_tile[MMAX], q_keep[MMAX];
  __shared__ float q_box[MMAX * 4];
  __shared__ int s_wave[DW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, L = C - 1;
  // scores and labels as detections_f32 computes them: one wave per row
  for (int row = wave; row < N; row += DW) {
    const float* x = logits + size_t(row) * C;
    const float x0 = lane < C ? x[lane] : -INFINITY, x1 = lane + 64 < C ? x[lane + 64] : -INFINITY;
    const float m = wave_max(fmaxf(x0, x1));
    const float e0 = lane < C ? expf(x0 - m) : 0.f, e1 = lane + 64 < C ? expf(x1 - m) : 0.f;
    const float sum = wave_sum(e0 + e1);
    float best = lane < L ? e0 / sum : -1.f;
    int idx = lane;
    const float p1 = lane + 64 < L ? e1 / sum : -1.f;
    if (p1 > best) best = p1, idx = lane + 64;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(idx, o);
      if (ob > best || (ob == best && oi < idx)) best = ob, idx = oi;
    }
    if (lane == 0) {
      s_score[row] = best;
      s_label[row] = idx;
    }
  }
  __syncthreads();
  // the order: thread i counts the candidates that precede row i (a strict total order, so ranks are distinct and
  // below the number of candidates, which every thread counts as well)
  const float si = tid < N ? s_score[tid] : 0.f;
  const bool cand = tid < N && si > thr;
  int rank = 0, ncand = 0;
  for (int j = 0; j < N; ++j) {
    const float sj = s_score[j];
    const bool cj = sj > thr;
    ncand += cj;
    rank += cj && (sj > si || (sj == si && j < tid));
  }
  if (cand) {
    const int b = tid / M;
    const float* bx = boxes + size_t(tid) * 4;
    const float cx = bx[0], cy = bx[1], hw = 0.5f * bx[2], hh = 0.5f * bx[3];
    const float oy = float(origins[2 * b]), ox = float(origins[2 * b + 1]);
    q_score[rank] = si;
    q_label[rank] = s_label[tid];
    q_tile[rank] = b;
    q_keep[rank] = 1;
    q_box[rank * 4 + 0] = (cx - hw) * tw + ox;
    q_box[rank * 4 + 1] = (cy - hh) * th + oy;
    q_box[rank * 4 + 2] = (cx + hw) * tw + ox;
    q_box[rank * 4 + 3] = (cy + hh) * th + oy;
  }
  __syncthreads();
  // the greedy pass: thread k owns candidate k; pivot p, when still kept, drops the later candidates it matches.
  // q_keep[k] is written by thread k alone and read as a pivot only after the barrier of a later iteration.
  const int k = tid;
  bool keep = k < ncand;
  float mine[4] = {0.f, 0.f, 0.f, 0.f};
  int lab = -1, tl = -1;
  if (keep) {
#pragma unroll
    for (int c = 0; c < 4; ++c) mine[c] = q_box[k * 4 + c];
    lab = q_label[k], tl = q_tile[k];
  }
  for (int p = 0; p + 1 < ncand; ++p) {
    __syncthreads();
    if (!q_keep[p]) continue;  // the same in every thread
    if (keep && k > p && q_label[p] == lab && q_tile[p] != tl && box_overlap(q_box + p * 4, mine, iou) > mt) {
      keep = false;
      q_keep[k] = 0;
    }
  }
  __syncthreads();
  // the kept candidates, in order, to the front
  const unsigned long long mask = __ballot(keep);
  if (lane == 0) s_wave[wave] = __popcll(mask);
  __syncthreads();
  int off = 0, total = 0;
  for (int w = 0; w < DW; ++w) {
    off += w < wave ? s_wave[w] : 0;
    total += s_wave[w];
  }
  if (keep) {
    const int slot = off + __popcll(mask & ((1ull << lane) - 1ull));
    scores[slot] = q_score[k];
    labels[slot] = lab;
    tile[slot] = tl;
#pragma unroll
    for (int c = 0; c < 4; ++c) out_boxes[slot * 4 + c] = mine[c];
  }
  for (int z = total + tid; z < N; z += DT) {
    scores[z] = 0.f;
    labels[z] = 0;
    tile[z] = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) out_boxes[z * 4 + c] = 0.f;
  }
  if (tid == 0) count[0] = total;
}

int check(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return int(e);
  }
  return 0;
}

int fail(const char* msg) {
  g_err = msg;
  return -1;
}
// what both image entries check and fill (all but the source); grid: the workgroups to launch
int image_args(ImgArgs& k, int& grid, void* planes, float* pixels, const int* yidx, const float* ywt, const int* xidx,
               const float* xwt, int ytab, int xtab, int taps, int max_fh, int max_fw, const float* a, const float* b,
               int B, int h, int w, int H, int W, int p, int gh, int gw, int wgs) {
  if (!planes || !yidx || !ywt || !xidx || !xwt || !a || !b) return fail("image_patch_planes: null operand");
  if (B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return fail("image_patch_planes: B, h, w, H, W must be positive");
  if (p < 2 || p % 2 || p > PMAX) return fail("image_patch_planes: patch side must be even and at most 16");
  if (gh <= 0 || gw <= 0 || size_t(gh) * p > size_t(H) || size_t(gw) * p > size_t(W))
    return fail("image_patch_planes: whole patches inside the resized image (gh * p <= H, gw * p <= W)");
  if (taps != TAPS || ytab != H || xtab != W) return fail("image_patch_planes: tap tables must be [H][9] and [W][9]");
  if (max_fh <= 0 || max_fw <= 0 || max_fh > FMAX || max_fw > FMAX || max_fh > h || max_fw > w)
    return fail("image_patch_planes: a patch's source footprint exceeds 72 rows or columns (scale above 4)");
  k.planes = static_cast<__bf16*>(planes);
  k.pixels = pixels;
  k.yidx = yidx, k.ywt = ywt, k.xidx = xidx, k.xwt = xwt;
  for (int c = 0; c < 3; ++c) k.a[c] = a[c], k.b[c] = b[c];
  k.B = B, k.h = h, k.w = w, k.H = H, k.W = W, k.p = p, k.gh = gh, k.gw = gw;
  // with pixels every tile that covers H x W is computed; without, only the patch grid
  k.GH = pixels ? (H + p - 1) / p : gh;
  k.GW = pixels ? (W + p - 1) / p : gw;
  const size_t tiles = size_t(B) * k.GH * k.GW;
  if (tiles > size_t(1) << 30) return fail("image_patch_planes: too many patches");
  grid = int(wgs > 0 && size_t(wgs) < tiles ? size_t(wgs) : tiles);
  return 0;
}

// a plane of B x rows x rowbytes at ptr (batch stride bs, possibly negative; row pitch) lies inside [lo, hi)
bool inside(int B, const void* ptr, const void* lo, const void* hi, long long bs, long long rows, long long pitch,
            long long rowbytes) {
  const long long first = std::min(0LL, (B - 1) * bs), last = std::max(0LL, (B - 1) * bs) + (rows - 1) * pitch + rowbytes;
  const intptr_t q = reinterpret_cast<intptr_t>(ptr);
  return lo && hi && q + first >= reinterpret_cast<intptr_t>(lo) && q + last <= reinterpret_cast<intptr_t>(hi);
}

bool stride_range(long long pitch, long long bs) { return std::llabs(bs) <= (1LL << 40) && pitch <= (1LL << 30); }

bool table_ok(const int* table) {
  for (int i = 0; i < 12; ++i)
    if (i < 9 ? std::abs(table[i]) >= (1 << 23) : (table[i] < 0 || table[i] > 255)) return false;
  return true;
}

PlaneArg plane_arg(const void* p, const void* lo, const void* hi, long long pitch, long long bs) {
  return PlaneArg{static_cast<const uint8_t*>(p), reinterpret_cast<uintptr_t>(lo), reinterpret_cast<uintptr_t>(hi), pitch,
                  bs};
}

// both orders of the semi-planar entry: vu = 0 is NV12 (U, V), 1 is NV21 (V, U)
int patch_planes_semiplanar(const void* y, const void* y_lo, const void* y_hi, const void* uv, const void* uv_lo,
                            const void* uv_hi, long long y_pitch, long long uv_pitch, long long y_bstride,
                            long long uv_bstride, const int* table, void* planes, float* pixels, const int* yidx,
                            const float* ywt, const int* xidx, const float* xwt, int ytab, int xtab, int taps,
                            int max_fh, int max_fw, const float* a, const float* b, int B, int h, int w, int H, int W,
                            int p, int gh, int gw, int wgs, void* stream, int vu) {
  if (!y || !uv || !table) return fail("image_patch_planes: null operand");
  if (vu != 0 && vu != 1) return fail("image_patch_planes_nv12: the chroma order is 0 (U, V) or 1 (V, U)");
  ImgArgs k{};
  int grid = 0;
  if (const int rc = image_args(k, grid, planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b,
                                B, h, w, H, W, p, gh, gw, wgs))
    return rc;
  if (max_fw > NV12_FMAX_W) return fail("image_patch_planes_nv12: a patch's source footprint exceeds 69 columns");
  const long long ch = (h + 1) / 2, cw2 = 2 * ((w + 1) / 2LL);
  if (y_pitch < w) return fail("image_patch_planes_nv12: the Y pitch is smaller than the width");
  if (uv_pitch < cw2) return fail("image_patch_planes_nv12: the UV pitch is smaller than 2 * ((w + 1) / 2)");
  if (!stride_range(y_pitch, y_bstride) || !stride_range(uv_pitch, uv_bstride))
    return fail("image_patch_planes_nv12: pitch or batch stride out of range");
  // the planes' first and one-past-last byte (a batch stride may be negative) inside the storage
  if (!inside(B, y, y_lo, y_hi, y_bstride, h, y_pitch, w) || !inside(B, uv, uv_lo, uv_hi, uv_bstride, ch, uv_pitch, cw2))
    return fail("image_patch_planes_nv12: a plane does not lie inside its storage bounds");
  if (!table_ok(table))
    return fail("image_patch_planes_nv12: colour table: coefficients below 2^23 in size, offsets in 0..255");
  Nv12Args n{};
  n.y = static_cast<const uint8_t*>(y), n.uv = static_cast<const uint8_t*>(uv);
  n.ylo = reinterpret_cast<uintptr_t>(y_lo), n.yhi = reinterpret_cast<uintptr_t>(y_hi);
  n.uvlo = reinterpret_cast<uintptr_t>(uv_lo), n.uvhi = reinterpret_cast<uintptr_t>(uv_hi);
  n.ypitch = y_pitch, n.uvpitch = uv_pitch, n.ybs = y_bstride, n.uvbs = uv_bstride;
  for (int i = 0; i < 12; ++i) n.tab[i] = table[i];
  hipLaunchKernelGGL(vu ? image_patch_planes_nv21 : image_patch_planes_nv12, dim3(grid), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), k, n);
  return check(vu ? "image_patch_planes_nv21" : "image_patch_planes_nv12");
}
// What the entries of the general YUV front end check and fill: every check of the descriptor and of the common
// arguments, then the kernel's arguments k and n and the workgroups to launch. sB x sh x sw: the batch and the size
// of the source the descriptor's planes hold — B x h x w itself, or the one frame that B tiles of h x w are cut from.
int yuv_args(const NosYuvSrc* src, ImgArgs& k, int& grid, YuvBilinearArgs& n, void* planes, float* pixels,
             const int* yidx, const float* ywt, const int* xidx, const float* xwt, int ytab, int xtab, int taps,
             int max_fh, int max_fw, const float* a, const float* b, int B, int h, int w, int H, int W, int p, int gh,
             int gw, int wgs, int sB, int sh, int sw) {
  if (!src) return fail("image_patch_planes: null operand");
  if (src->size != int(sizeof(NosYuvSrc)))
    return fail("image_patch_planes_yuv: descriptor size mismatch (NosYuvSrc of another build)");
  const NosYuvSrc& s = *src;
  if (const int rc = image_args(k, grid, planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b,
                                B, h, w, H, W, p, gh, gw, wgs))
    return rc;
  if (max_fw > YUV_FMAX_W) return fail("image_patch_planes_yuv: a patch's source footprint exceeds 69 columns");
  // the known combinations
  const bool packed = s.layout == YUV_PACKED;
  if (s.layout != YUV_PLANAR && s.layout != YUV_SEMI && !packed)
    return fail("image_patch_planes_yuv: unknown layout (0 planar, 1 semi-planar, 2 packed 4:2:2)");
  if (!((s.hsub == 1 && s.vsub == 1) || (s.hsub == 1 && s.vsub == 0) || (s.hsub == 0 && s.vsub == 0)))
    return fail("image_patch_planes_yuv: unknown subsampling (hsub, vsub): (1, 1), (1, 0) or (0, 0)");
  if (packed && (s.hsub != 1 || s.vsub != 0 || s.sample_bytes != 1))
    return fail("image_patch_planes_yuv: packed sources are 4:2:2 with 8-bit samples");
  if (s.sample_bytes == 1 ? (s.depth != 8 || s.shift != 0)
                          : (s.sample_bytes != 2 || (s.depth != 10 && s.depth != 12) ||
                             (s.shift != 0 && s.shift != 16 - s.depth)))
    return fail("image_patch_planes_yuv: unknown sample format (1 byte: depth 8, shift 0; 2 bytes: depth 10 or 12, "
                "shift 0 or 16 - depth)");
  if (s.order < 0 || s.order > (packed ? 2 : s.layout == YUV_SEMI ? 1 : 0))
    return fail("image_patch_planes_yuv: unknown order (semi-planar 0 UV / 1 VU; packed 0 YUYV / 1 UYVY / 2 YVYU)");
  if (s.chroma != 0 && s.chroma != 1)
    return fail("image_patch_planes_yuv: unknown chroma reconstruction (0 nearest, 1 bilinear)");
  if (s.siting < 0 || s.siting > 3)
    return fail("image_patch_planes_yuv: unknown chroma siting (bit 0 horizontally, bit 1 vertically co-sited)");
  if (s.chroma == 1 && s.hsub == 0)
    return fail("image_patch_planes_yuv: bilinear chroma takes a subsampled source (4:4:4 is launched as nearest)");
  // rows and row bytes of every plane
  const long long SB = s.sample_bytes, cw = (sw + (1LL << s.hsub) - 1) >> s.hsub,
                  ch = (sh + (1LL << s.vsub) - 1) >> s.vsub;
  const int np = packed ? 1 : s.layout == YUV_SEMI ? 2 : 3;
  const long long rows[3] = {sh, ch, ch};
  const long long rowbytes[3] = {packed ? 4 * ((sw + 1LL) / 2) : sw * SB, s.layout == YUV_SEMI ? 2 * cw * SB : cw * SB,
                                 cw * SB};
  for (int i = 0; i < np; ++i) {
    const NosYuvPlane& q = s.plane[i];
    if (!q.p) return fail("image_patch_planes: null operand");
    if (q.pitch < rowbytes[i]) return fail("image_patch_planes_yuv: a plane's pitch is smaller than its row's bytes");
    if (!stride_range(q.pitch, q.bstride)) return fail("image_patch_planes_yuv: pitch or batch stride out of range");
    if (SB == 2 && ((reinterpret_cast<uintptr_t>(q.p) | uintptr_t(q.pitch) | uintptr_t(q.bstride)) & 1))
      return fail("image_patch_planes_yuv: 16-bit planes lie at an even address with an even pitch and batch stride");
    if (!inside(sB, q.p, q.lo, q.hi, q.bstride, rows[i], q.pitch, rowbytes[i]))
      return fail("image_patch_planes_yuv: a plane does not lie inside its storage bounds");
    n.pl[i] = plane_arg(q.p, q.lo, q.hi, q.pitch, q.bstride);
  }
  for (int i = 0; i < 12; ++i) {
    if (i < 9 ? std::abs(s.tab[i]) >= (1 << 23) : (s.tab[i] < 0 || s.tab[i] >= (1 << s.depth)))
      return fail("image_patch_planes_yuv: colour table: coefficients below 2^23 in size, offsets below 2^depth");
    n.tab[i] = s.tab[i];
  }
  n.vsub = s.vsub, n.depth = s.depth, n.shift = s.shift, n.mask = (1 << s.depth) - 1, n.order = s.order;
  // co-sited: (4, 0) of C[i], C[i] at an even position, held as (0, 4) of C[i - 1], C[i], and (2, 2) at an odd one;
  // centred: (1, 3) and (3, 1)
  n.cw = int(cw), n.ch = int(ch);
  static const int cosited[4] = {0, 4, 2, 2}, centred[4] = {1, 3, 3, 1};
  for (int i = 0; i < 4; ++i)
    n.wx[i] = (s.siting & 1 ? cosited : centred)[i], n.wy[i] = (s.siting & 2 ? cosited : centred)[i];
  return 0;
}

// What both HDR entries check of the tables (after yuv_args) and fill of n.
int hdr_args(const NosYuvSrc& s, const NosYuvHdr& hdr, YuvHdrArgs& n) {
  if (s.sample_bytes != 2 || s.layout == YUV_PACKED)
    return fail("image_patch_planes_yuv_hdr: a source of 16-bit samples (depth 10 or 12), planar or semi-planar");
  if (hdr.entries != 1 << s.depth) return fail("image_patch_planes_yuv_hdr: lut1 has 2^depth entries");
  if (!hdr.lut1 || !hdr.lut2) return fail("image_patch_planes_yuv_hdr: null table");
  for (int i = 0; i < 9; ++i) {
    if (std::abs(hdr.gamut[i]) >= (1 << 15))
      return fail("image_patch_planes_yuv_hdr: gamut coefficients below 2^15 in size");
    n.gamut[i] = hdr.gamut[i];
  }
  n.lut1 = static_cast<const uint16_t*>(hdr.lut1), n.lut2 = static_cast<const uint8_t*>(hdr.lut2);
  n.entries = hdr.entries;
  return 0;
}
}  // namespace

extern "C" {

const char* nos_image_last_error() { return g_err.c_str(); }

int nos_image_taps() { return TAPS; }
int nos_image_max_footprint() { return FMAX; }
int nos_image_max_patch() { return PMAX; }

int nos_image_nv12_max_footprint() { return NV12_FMAX_W; }
int nos_image_yuv420p_max_footprint() { return YUV420P_FMAX_W; }
int nos_image_packed_max_footprint() { return PACKED_FMAX_W; }

// img [B][h][w][3] uint8 -> planes [3][B*gh*gw][3*p*p] bf16 (and pixels [B][3][H][W] fp32 when
// non-null). yidx [2][H] / xidx [2][W] (first source index, tap count) and ywt [H][taps] / xwt
// [W][taps] are device tables; ytab / xtab are their row counts, max_fh / max_fw the largest source
// footprint of one patch row / column of those tables (the host built them, so it knows). a, b:
// host arrays of the three per-channel affine constants. wgs: workgroups (0 = one per tile).
int nos_image_patch_planes_u8(const void* img, void* planes, float* pixels, const int* yidx, const float* ywt,
                              const int* xidx, const float* xwt, int ytab, int xtab, int taps, int max_fh, int max_fw,
                              const float* a, const float* b, int B, int h, int w, int H, int W, int p, int gh, int gw,
                              int wgs, void* stream) {
  if (!img) return fail("image_patch_planes: null operand");
  ImgArgs k{};
  int grid = 0;
  if (const int rc = image_args(k, grid, planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b,
                                B, h, w, H, W, p, gh, gw, wgs))
    return rc;
  k.img = static_cast<const uint8_t*>(img);
  hipLaunchKernelGGL(image_patch_planes_u8, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k);
  return check("image_patch_planes_u8");
}

// The same from an NV12 frame: y [B][h][w] uint8 with row pitch y_pitch and batch stride y_bstride
// (bytes), uv [B][(h+1)/2][(w+1)/2][2] uint8 (U, V) with uv_pitch and uv_bstride; [y_lo, y_hi) and
// [uv_lo, uv_hi) are the first and one-past-last byte of the storage each plane lives in (the kernel
// reads whole dwords where it can, and never outside them). table: 12 host integers, the 3 x 3 colour
// matrix in 16.16 fixed point by rows (R, G, B) x (Y, U, V), each below 2^23 in size, then the offsets
// of Y, U and V (0..255). The rest as nos_image_patch_planes_u8.
int nos_image_patch_planes_nv12(const void* y, const void* y_lo, const void* y_hi, const void* uv, const void* uv_lo,
                                const void* uv_hi, long long y_pitch, long long uv_pitch, long long y_bstride,
                                long long uv_bstride, const int* table, void* planes, float* pixels, const int* yidx,
                                const float* ywt, const int* xidx, const float* xwt, int ytab, int xtab, int taps,
                                int max_fh, int max_fw, const float* a, const float* b, int B, int h, int w, int H, int W,
                                int p, int gh, int gw, int wgs, void* stream) {
  return patch_planes_semiplanar(y, y_lo, y_hi, uv, uv_lo, uv_hi, y_pitch, uv_pitch, y_bstride, uv_bstride, table, planes,
                                 pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b, B, h, w, H, W, p,
                                 gh, gw, wgs, stream, 0);
}

// nos_image_patch_planes_nv12 with the order of a chroma pair as a trailing argument: vu = 0 for NV12 (U, V),
// 1 for NV21 (V, U).
int nos_image_patch_planes_nv12_order(const void* y, const void* y_lo, const void* y_hi, const void* uv,
                                      const void* uv_lo, const void* uv_hi, long long y_pitch, long long uv_pitch,
                                      long long y_bstride, long long uv_bstride, const int* table, void* planes,
                                      float* pixels, const int* yidx, const float* ywt, const int* xidx,
                                      const float* xwt, int ytab, int xtab, int taps, int max_fh, int max_fw,
                                      const float* a, const float* b, int B, int h, int w, int H, int W, int p, int gh,
                                      int gw, int wgs, void* stream, int vu) {
  return patch_planes_semiplanar(y, y_lo, y_hi, uv, uv_lo, uv_hi, y_pitch, uv_pitch, y_bstride, uv_bstride, table, planes,
                                 pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b, B, h, w, H, W, p,
                                 gh, gw, wgs, stream, vu);
}

// The same from planar 4:2:0: y [B][h][w], u and v [B][(h+1)/2][(w+1)/2] uint8, each plane with its own row
// pitch, batch stride (bytes) and storage bounds as in nos_image_patch_planes_nv12 (YV12: pass the planes by
// what they hold, not by where they lie). table and the rest as there.
int nos_image_patch_planes_yuv420p(const void* y, const void* y_lo, const void* y_hi, const void* u, const void* u_lo,
                                   const void* u_hi, const void* v, const void* v_lo, const void* v_hi,
                                   long long y_pitch, long long u_pitch, long long v_pitch, long long y_bstride,
                                   long long u_bstride, long long v_bstride, const int* table, void* planes,
                                   float* pixels, const int* yidx, const float* ywt, const int* xidx, const float* xwt,
                                   int ytab, int xtab, int taps, int max_fh, int max_fw, const float* a, const float* b,
                                   int B, int h, int w, int H, int W, int p, int gh, int gw, int wgs, void* stream) {
  if (!y || !u || !v || !table) return fail("image_patch_planes: null operand");
  ImgArgs k{};
  int grid = 0;
  if (const int rc = image_args(k, grid, planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b,
                                B, h, w, H, W, p, gh, gw, wgs))
    return rc;
  if (max_fw > YUV420P_FMAX_W) return fail("image_patch_planes_yuv420p: a patch's source footprint exceeds 69 columns");
  const long long ch = (h + 1) / 2, cw = (w + 1) / 2;
  if (y_pitch < w) return fail("image_patch_planes_yuv420p: the Y pitch is smaller than the width");
  if (u_pitch < cw) return fail("image_patch_planes_yuv420p: the U pitch is smaller than (w + 1) / 2");
  if (v_pitch < cw) return fail("image_patch_planes_yuv420p: the V pitch is smaller than (w + 1) / 2");
  if (!stride_range(y_pitch, y_bstride) || !stride_range(u_pitch, u_bstride) || !stride_range(v_pitch, v_bstride))
    return fail("image_patch_planes_yuv420p: pitch or batch stride out of range");
  if (!inside(B, y, y_lo, y_hi, y_bstride, h, y_pitch, w) || !inside(B, u, u_lo, u_hi, u_bstride, ch, u_pitch, cw) ||
      !inside(B, v, v_lo, v_hi, v_bstride, ch, v_pitch, cw))
    return fail("image_patch_planes_yuv420p: a plane does not lie inside its storage bounds");
  if (!table_ok(table))
    return fail("image_patch_planes_yuv420p: colour table: coefficients below 2^23 in size, offsets in 0..255");
  PlanarArgs n{};
  n.y = plane_arg(y, y_lo, y_hi, y_pitch, y_bstride);
  n.u = plane_arg(u, u_lo, u_hi, u_pitch, u_bstride);
  n.v = plane_arg(v, v_lo, v_hi, v_pitch, v_bstride);
  for (int i = 0; i < 12; ++i) n.tab[i] = table[i];
  hipLaunchKernelGGL(image_patch_planes_yuv420p, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k, n);
  return check("image_patch_planes_yuv420p");
}

// The same from packed pixels: img [B][h][w][C] uint8 with row pitch and batch stride in bytes (any pitch >=
// w * C, any alignment of the first byte, the batch stride possibly negative) inside the storage [lo, hi).
// order: "rgb", "bgr" (C = 3), "rgba" or "bgra" (C = 4; the fourth byte is never read as colour). A crop or
// a padded capture buffer is read in place. The rest as nos_image_patch_planes_u8.
int nos_image_patch_planes_packed(const void* img, const void* lo, const void* hi, long long pitch, long long bstride,
                                  const char* order, void* planes, float* pixels, const int* yidx, const float* ywt,
                                  const int* xidx, const float* xwt, int ytab, int xtab, int taps, int max_fh,
                                  int max_fw, const float* a, const float* b, int B, int h, int w, int H, int W, int p,
                                  int gh, int gw, int wgs, void* stream) {
  if (!img || !order) return fail("image_patch_planes: null operand");
  const std::string o(order);
  if (o != "rgb" && o != "bgr" && o != "rgba" && o != "bgra")
    return fail("image_patch_planes_packed: unknown channel order (rgb, bgr, rgba or bgra)");
  const int C = int(o.size());
  ImgArgs k{};
  int grid = 0;
  if (const int rc = image_args(k, grid, planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b,
                                B, h, w, H, W, p, gh, gw, wgs))
    return rc;
  if (max_fw > PACKED_FMAX_W) return fail("image_patch_planes_packed: a patch's source footprint exceeds 69 columns");
  if (pitch < (long long)w * C) return fail("image_patch_planes_packed: the row pitch is smaller than a row's bytes");
  if (!stride_range(pitch, bstride)) return fail("image_patch_planes_packed: pitch or batch stride out of range");
  if (!inside(B, img, lo, hi, bstride, h, pitch, (long long)w * C))
    return fail("image_patch_planes_packed: the image does not lie inside its storage bounds");
  PackedArgs n{};
  n.s = plane_arg(img, lo, hi, pitch, bstride);
  n.r = o[0] == 'r' ? 0 : 2, n.g = 1, n.b = 2 - n.r;
  if (C == 4)
    hipLaunchKernelGGL(image_patch_planes_packed4, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k, n);
  else
    hipLaunchKernelGGL(image_patch_planes_packed3, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k, n);
  return check("image_patch_planes_packed");
}

// B tiles of tile_h x tile_w pixels (h and w of the common arguments) of one packed frame img [frame_h][frame_w][C]
// (order, pitch, [lo, hi) as in nos_image_patch_planes_packed), as that entry gives for the B crops stacked. origins:
// host array [B][2] of every tile's first row and column; table: device array [B] of int64 byte offsets from img,
// origins[b][0] * pitch + origins[b][1] * C (the host built both from one plan; a graph holds the table). Nothing is
// launched unless the frame lies inside its storage and every tile inside the frame; the kernel reads no byte outside
// [lo, hi) whatever the table holds.
int nos_image_patch_planes_tiles(const void* img, const void* lo, const void* hi, long long pitch, const char* order,
                                 const int* origins, const long long* table, int frame_h, int frame_w, void* planes,
                                 float* pixels, const int* yidx, const float* ywt, const int* xidx, const float* xwt,
                                 int ytab, int xtab, int taps, int max_fh, int max_fw, const float* a, const float* b,
                                 int B, int h, int w, int H, int W, int p, int gh, int gw, int wgs, void* stream) {
  if (!img || !order) return fail("image_patch_planes: null operand");
  if (!origins || !table) return fail("image_patch_planes_tiles: null origin table");
  const std::string o(order);
  if (o != "rgb" && o != "bgr" && o != "rgba" && o != "bgra")
    return fail("image_patch_planes_tiles: unknown channel order (rgb, bgr, rgba or bgra)");
  const int C = int(o.size());
  ImgArgs k{};
  int grid = 0;
  if (const int rc = image_args(k, grid, planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b,
                                B, h, w, H, W, p, gh, gw, wgs))
    return rc;
  if (max_fw > PACKED_FMAX_W) return fail("image_patch_planes_tiles: a patch's source footprint exceeds 69 columns");
  if (frame_h <= 0 || frame_w <= 0) return fail("image_patch_planes_tiles: the frame's sizes must be positive");
  if (pitch < (long long)frame_w * C) return fail("image_patch_planes_tiles: the row pitch is smaller than a row's bytes");
  if (!stride_range(pitch, 0)) return fail("image_patch_planes_tiles: pitch out of range");
  if (!inside(1, img, lo, hi, 0, frame_h, pitch, (long long)frame_w * C))
    return fail("image_patch_planes_tiles: the frame does not lie inside its storage bounds");
  for (int t = 0; t < B; ++t) {
    const long long y0 = origins[2 * t], x0 = origins[2 * t + 1];
    if (y0 < 0 || x0 < 0 || y0 + h > frame_h || x0 + w > frame_w)
      return fail("image_patch_planes_tiles: a tile does not lie inside the frame");
  }
  PackedTileArgs n{};
  n.s = plane_arg(img, lo, hi, pitch, 0);
  n.r = o[0] == 'r' ? 0 : 2, n.g = 1, n.b = 2 - n.r;
  n.origin = table;
  if (C == 4)
    hipLaunchKernelGGL(image_patch_planes_tiles4, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k, n);
  else
    hipLaunchKernelGGL(image_patch_planes_tiles3, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k, n);
  return check("image_patch_planes_tiles");
}

int nos_image_yuv_max_footprint() { return YUV_FMAX_W; }

// The same from any YUV surface NosYuvSrc (image_yuv.h) describes: planar, semi-planar or packed 4:2:2; 4:2:0,
// 4:2:2 or 4:4:4; 8-bit samples or 10 / 12-bit codes in little-endian 16-bit words (in the high or the low bits;
// the other bits are ignored, not required to be zero). Nothing is launched unless every check passes.
int nos_image_patch_planes_yuv(const NosYuvSrc* src, void* planes, float* pixels, const int* yidx, const float* ywt,
                               const int* xidx, const float* xwt, int ytab, int xtab, int taps, int max_fh, int max_fw,
                               const float* a, const float* b, int B, int h, int w, int H, int W, int p, int gh, int gw,
                               int wgs, void* stream) {
  ImgArgs k{};
  int grid = 0;
  YuvBilinearArgs n{};
  if (const int rc = yuv_args(src, k, grid, n, planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a,
                              b, B, h, w, H, W, p, gh, gw, wgs, B, h, w))
    return rc;
  const NosYuvSrc& s = *src;
  if (s.chroma == 1) {
    // hsub is 1; packed sources have one sample size
    void (*bilinear)(ImgArgs, YuvBilinearArgs) = nullptr;
    switch (s.layout * 2 + (s.sample_bytes - 1)) {
      case 0: bilinear = image_patch_planes_yuv_bilinear<Yuv<YUV_PLANAR, 1, 1, 1>>; break;
      case 1: bilinear = image_patch_planes_yuv_bilinear<Yuv<YUV_PLANAR, 1, 2, 1>>; break;
      case 2: bilinear = image_patch_planes_yuv_bilinear<Yuv<YUV_SEMI, 1, 1, 1>>; break;
      case 3: bilinear = image_patch_planes_yuv_bilinear<Yuv<YUV_SEMI, 1, 2, 1>>; break;
      default: bilinear = image_patch_planes_yuv_bilinear<Yuv<YUV_PACKED, 1, 1, 1>>; break;
    }
    hipLaunchKernelGGL(bilinear, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k, n);
    return check("image_patch_planes_yuv");
  }
  void (*kern)(ImgArgs, YuvArgs) = nullptr;
  switch (s.layout * 4 + s.hsub * 2 + (s.sample_bytes - 1)) {
    case 0: kern = image_patch_planes_yuv<Yuv<YUV_PLANAR, 0, 1>>; break;
    case 1: kern = image_patch_planes_yuv<Yuv<YUV_PLANAR, 0, 2>>; break;
    case 2: kern = image_patch_planes_yuv<Yuv<YUV_PLANAR, 1, 1>>; break;
    case 3: kern = image_patch_planes_yuv<Yuv<YUV_PLANAR, 1, 2>>; break;
    case 4: kern = image_patch_planes_yuv<Yuv<YUV_SEMI, 0, 1>>; break;
    case 5: kern = image_patch_planes_yuv<Yuv<YUV_SEMI, 0, 2>>; break;
    case 6: kern = image_patch_planes_yuv<Yuv<YUV_SEMI, 1, 1>>; break;
    case 7: kern = image_patch_planes_yuv<Yuv<YUV_SEMI, 1, 2>>; break;
    default: kern = image_patch_planes_yuv<Yuv<YUV_PACKED, 1, 1>>; break;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k, YuvArgs(n));
  return check("image_patch_planes_yuv");
}

// The same of a source whose codes are PQ or HLG, through the tables NosYuvHdr (image_yuv.h) points to: 10 / 12-bit
// codes in 16-bit words, planar or semi-planar, nearest or bilinear chroma. Every check of nos_image_patch_planes_yuv,
// then those of the tables; nothing is launched unless all pass.
int nos_image_patch_planes_yuv_hdr(const NosYuvSrc* src, const NosYuvHdr* hdr, void* planes, float* pixels,
                                   const int* yidx, const float* ywt, const int* xidx, const float* xwt, int ytab,
                                   int xtab, int taps, int max_fh, int max_fw, const float* a, const float* b, int B,
                                   int h, int w, int H, int W, int p, int gh, int gw, int wgs, void* stream) {
  if (!hdr) return fail("image_patch_planes: null operand");
  if (hdr->size != int(sizeof(NosYuvHdr)))
    return fail("image_patch_planes_yuv_hdr: table descriptor size mismatch (NosYuvHdr of another build)");
  ImgArgs k{};
  int grid = 0;
  YuvHdrArgs n{};
  if (const int rc = yuv_args(src, k, grid, n, planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a,
                              b, B, h, w, H, W, p, gh, gw, wgs, B, h, w))
    return rc;
  const NosYuvSrc& s = *src;
  if (const int rc = hdr_args(s, *hdr, n)) return rc;
  void (*kern)(ImgArgs, YuvHdrArgs) = nullptr;
  switch ((s.layout == YUV_SEMI ? 3 : 0) + (s.chroma == 1 ? 2 : s.hsub)) {
    case 0: kern = image_patch_planes_yuv_hdr<Yuv<YUV_PLANAR, 0, 2>>; break;
    case 1: kern = image_patch_planes_yuv_hdr<Yuv<YUV_PLANAR, 1, 2>>; break;
    case 2: kern = image_patch_planes_yuv_hdr<Yuv<YUV_PLANAR, 1, 2, 1>>; break;
    case 3: kern = image_patch_planes_yuv_hdr<Yuv<YUV_SEMI, 0, 2>>; break;
    case 4: kern = image_patch_planes_yuv_hdr<Yuv<YUV_SEMI, 1, 2>>; break;
    default: kern = image_patch_planes_yuv_hdr<Yuv<YUV_SEMI, 1, 2, 1>>; break;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k, n);
  return check("image_patch_planes_yuv_hdr");
}

// B tiles of tile_h x tile_w pixels (h and w of the common arguments) of one YUV frame of frame_h x frame_w, as
// nos_image_patch_planes_yuv (hdr null) or nos_image_patch_planes_yuv_hdr gives for the B crops of the converted frame
// stacked. src describes the frame's planes; frames is the batch they hold, which must be 1. origins: host array
// [B][2] of every tile's first row and column; table: the same as a device array of int32 (a graph holds it; it is
// the one nos_merge_detections_f32 reads). Every check of those entries against the frame's size; nothing is launched
// unless they pass and every tile lies inside the frame. The kernel skips a patch that the table moves out of the
// frame, and reads no byte outside a plane's [lo, hi) whatever the table holds.
int nos_image_patch_planes_yuv_tiles(const NosYuvSrc* src, const NosYuvHdr* hdr, const int* origins, const int* table,
                                     int frame_h, int frame_w, int frames, void* planes, float* pixels,
                                     const int* yidx, const float* ywt, const int* xidx, const float* xwt, int ytab,
                                     int xtab, int taps, int max_fh, int max_fw, const float* a, const float* b, int B,
                                     int h, int w, int H, int W, int p, int gh, int gw, int wgs, void* stream) {
  if (!origins || !table) return fail("image_patch_planes_yuv_tiles: null origin table");
  if (frames != 1) return fail("image_patch_planes_yuv_tiles: tiles are cut from one frame (a source batch of 1)");
  if (frame_h <= 0 || frame_w <= 0) return fail("image_patch_planes_yuv_tiles: the frame's sizes must be positive");
  if (hdr && hdr->size != int(sizeof(NosYuvHdr)))
    return fail("image_patch_planes_yuv_hdr: table descriptor size mismatch (NosYuvHdr of another build)");
  ImgArgs k{};
  int grid = 0;
  YuvHdrTileArgs n{};
  if (const int rc = yuv_args(src, k, grid, n, planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a,
                              b, B, h, w, H, W, p, gh, gw, wgs, 1, frame_h, frame_w))
    return rc;
  const NosYuvSrc& s = *src;
  if (hdr)
    if (const int rc = hdr_args(s, *hdr, n)) return rc;
  for (int t = 0; t < B; ++t) {
    const long long y0 = origins[2 * t], x0 = origins[2 * t + 1];
    if (y0 < 0 || x0 < 0 || y0 + h > frame_h || x0 + w > frame_w)
      return fail("image_patch_planes_yuv_tiles: a tile does not lie inside the frame");
  }
  n.f = TileFrame{table, frame_h, frame_w};
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hdr) {
    void (*kern)(ImgArgs, YuvHdrTileArgs) = nullptr;
    switch ((s.layout == YUV_SEMI ? 3 : 0) + (s.chroma == 1 ? 2 : s.hsub)) {
      case 0: kern = image_patch_planes_yuv_hdr_tiles<Yuv<YUV_PLANAR, 0, 2>>; break;
      case 1: kern = image_patch_planes_yuv_hdr_tiles<Yuv<YUV_PLANAR, 1, 2>>; break;
      case 2: kern = image_patch_planes_yuv_hdr_tiles<Yuv<YUV_PLANAR, 1, 2, 1>>; break;
      case 3: kern = image_patch_planes_yuv_hdr_tiles<Yuv<YUV_SEMI, 0, 2>>; break;
      case 4: kern = image_patch_planes_yuv_hdr_tiles<Yuv<YUV_SEMI, 1, 2>>; break;
      default: kern = image_patch_planes_yuv_hdr_tiles<Yuv<YUV_SEMI, 1, 2, 1>>; break;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, k, n);
    return check("image_patch_planes_yuv_tiles");
  }
  if (s.chroma == 1) {
    YuvBilinearTileArgs nb{};
    static_cast<YuvBilinearArgs&>(nb) = n;
    nb.f = n.f;
    void (*bilinear)(ImgArgs, YuvBilinearTileArgs) = nullptr;
    switch (s.layout * 2 + (s.sample_bytes - 1)) {
      case 0: bilinear = image_patch_planes_yuv_bilinear_tiles<Yuv<YUV_PLANAR, 1, 1, 1>>; break;
      case 1: bilinear = image_patch_planes_yuv_bilinear_tiles<Yuv<YUV_PLANAR, 1, 2, 1>>; break;
      case 2: bilinear = image_patch_planes_yuv_bilinear_tiles<Yuv<YUV_SEMI, 1, 1, 1>>; break;
      case 3: bilinear = image_patch_planes_yuv_bilinear_tiles<Yuv<YUV_SEMI, 1, 2, 1>>; break;
      default: bilinear = image_patch_planes_yuv_bilinear_tiles<Yuv<YUV_PACKED, 1, 1, 1>>; break;
    }
    hipLaunchKernelGGL(bilinear, dim3(grid), dim3(256), 0, st, k, nb);
    return check("image_patch_planes_yuv_tiles");
  }
  YuvTileArgs nn{};
  static_cast<YuvArgs&>(nn) = n;
  nn.f = n.f;
  void (*kern)(ImgArgs, YuvTileArgs) = nullptr;
  switch (s.layout * 4 + s.hsub * 2 + (s.sample_bytes - 1)) {
    case 0: kern = image_patch_planes_yuv_tiles<Yuv<YUV_PLANAR, 0, 1>>; break;
    case 1: kern = image_patch_planes_yuv_tiles<Yuv<YUV_PLANAR, 0, 2>>; break;
    case 2: kern = image_patch_planes_yuv_tiles<Yuv<YUV_PLANAR, 1, 1>>; break;
    case 3: kern = image_patch_planes_yuv_tiles<Yuv<YUV_PLANAR, 1, 2>>; break;
    case 4: kern = image_patch_planes_yuv_tiles<Yuv<YUV_SEMI, 0, 1>>; break;
    case 5: kern = image_patch_planes_yuv_tiles<Yuv<YUV_SEMI, 0, 2>>; break;
    case 6: kern = image_patch_planes_yuv_tiles<Yuv<YUV_SEMI, 1, 1>>; break;
    case 7: kern = image_patch_planes_yuv_tiles<Yuv<YUV_SEMI, 1, 2>>; break;
    default: kern = image_patch_planes_yuv_tiles<Yuv<YUV_PACKED, 1, 1>>; break;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, k, nn);
  return check("image_patch_planes_yuv_tiles");
}

// logits [B][M][C] fp32, boxes [B][M][4] fp32, target [B][2] fp32 (height, width), all on the device ->
// count [B] int32, scores [B][M] fp32, labels [B][M] int32, out_boxes [B][M][4] fp32
int nos_detections_f32(const float* logits, const float* boxes, const float* target, float threshold, int B, int M,
                       int C, int* count, float* scores, int* labels, float* out_boxes, void* stream) {
  if (!logits || !boxes || !target || !count || !scores || !labels || !out_boxes)
    return fail("detections: null operand");
  if (B <= 0 || M <= 0 || M > MMAX || C < 2 || C > CMAX)
    return fail("detections: B > 0, 0 < M <= 1024, 2 <= classes (with \"no object\") <= 128");
  hipLaunchKernelGGL(detections_f32, dim3(B), dim3(DT), 0, reinterpret_cast<hipStream_t>(stream), logits, boxes,
                     target, threshold, M, C, scores, labels, out_boxes, count);
  return check("detections_f32");
}

// The detections of B tiles of one frame merged (merge_detections_f32): logits [B][M][C] fp32, boxes [B][M][4] fp32,
// origins [B][2] int32 (first row, first column of tile b), all on the device; tile_h, tile_w: the tiles' size in
// pixels; iou: 0 compares inter / min(area) with match_threshold, 1 inter / union -> count [1] int32, scores [B*M] fp32,
// labels [B*M] int32, out_boxes [B*M][4] fp32 (frame pixels), tile [B*M] int32
int nos_merge_detections_f32(const float* logits, const float* boxes, const int* origins, float tile_h, float tile_w,
                             float threshold, float match_threshold, int iou, int B, int M, int C, int* count,
                             float* scores, int* labels, float* out_boxes, int* tile, void* stream) {
  if (!logits || !boxes || !origins || !count || !scores || !labels || !out_boxes || !tile)
    return fail("merge_detections: null operand");
  if (B <= 0 || M <= 0 || (long long)B * M > MMAX || C < 2 || C > CMAX)
    return fail("merge_detections: 0 < B * M <= 1024, 2 <= classes (with \"no object\") <= 128");
  if (iou != 0 && iou != 1) return fail("merge_detections: the match is 0 (ios) or 1 (iou)");
  hipLaunchKernelGGL(merge_detections_f32, dim3(1), dim3(DT), 0, reinterpret_cast<hipStream_t>(stream), logits, boxes,
                     origins, tile_h, tile_w, threshold, match_threshold, iou, B * M, M, C, scores, labels, out_boxes,
                     tile, count);
  return check("merge_detections_f32");
}

}  // extern "C"
