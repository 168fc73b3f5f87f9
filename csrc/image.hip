// The image half of the workload (YOLOS-small): the pixels in front of the model and the detections
// behind it, each as one launch with no host synchronisation.
//
//  * Sources (enum class Src). Every layout is one instantiation of one kernel, image_patch_planes_k<Src, source
//    arguments[, Yuv<...>]>: contiguous RGB; the 8-bit 4:2:0 layouts NV12, NV21 and planar; packed pixels of 3 or 4
//    bytes, as a batch or as B tiles of one frame; and the general YUV front end behind one descriptor (image_yuv.h),
//    nearest, bilinear or HDR, again as a batch or as tiles. yuv_kernel lists the front end's instantiations.
//  * Staging (image_stage.h). What differs per source is only how a patch's source footprint becomes RGB bytes in
//    the LDS tile: the argument structs, the reads that never leave a plane's storage, the colour functions, stage_yuv
//    and stage_yuv_bilinear.
//  * Shared passes (image_patch_planes_body). Behind the staging loop every source runs the same code: separable
//    antialiased triangle resample to H x W (tap tables built on the host in fp64 and read as constants), the
//    per-channel affine v * a_c + b_c, and the exact x3 split into the three bf16 planes [3][B*gh*gw][3*p*p] of the
//    patch matrix (row (b, i, j), column (c, u, v), as patch_planes_f32 in head.hip); optionally the fp32 pixels
//    [B][3][H][W] as well. So every layout is bit-equal to the RGB kernel on the converted frame.
//  * Detections (image_detect.h): detections_f32 and merge_detections_f32.
//  * Tracking (image_track.h): track_update_f32, the detections of successive frames associated in device state.
//  * Drawing (image_overlay.h): overlay_k, the detections painted into the frame's own planes — the one kernel here
//    that writes a surface.
//  * Entries. The extern "C" functions at the end check every argument of an outside caller, fill the kernel's
//    arguments and launch; the arguments all image entries share travel as one struct (Common).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "image_detect.h"
#include "image_track.h"
#include "image_stage.h"
#include "image_overlay.h"
#include "image_yuv.h"

namespace {
thread_local std::string g_err;

// TAPS: weights per output row / column (scale <= 4: 2 * 4 + 1); PMAX: patch side; FMAX: rows and
// columns of a patch's source footprint, at most scale * (p + 1) + 1 = 69 at scale 4 and p = 16
// (the host passes the largest footprint of the tables and it is checked against FMAX).
constexpr int TAPS = 9, PMAX = 16, FMAX = 72;
// a footprint row in LDS: the global row's bytes at its own alignment (0-3 bytes of lead-in), whole dwords
constexpr int NDW = (FMAX * 3 + 3 + 3) / 4, RS = NDW * 4;

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

// The source layouts, one instantiation of the body and of the kernel each. RGB: contiguous
// [B][h][w][3], staged as whole rows of aligned dwords, footprints of up to FMAX = 72 columns. Every other
// layout stages columns in groups of 4 (for 4:2:0 one dword of luma and the two chroma samples under it, for
// packed pixels 12 or 16 source bytes; three dwords of RGB out): NG groups fit a row of the LDS tile, and
// any GROUP_FMAX_W = 69 columns lie inside 18 consecutive groups wherever they start, so these layouts
// cover footprints of up to 69 columns (scale 4 at patch 16); the host falls back past that.
// YUV is the general front end (image_yuv.h): its staging loop is instantiated per Yuv<layout, hsub, sample bytes>.
// TILES3 / TILES4 / YUV_TILES: the packed and the YUV staging loops over B tiles of one frame.
enum class Src { RGB, NV12, NV21, YUV420P, PACKED3, PACKED4, YUV, TILES3, TILES4, YUV_TILES };
constexpr int NG = RS / 12, GROUP_FMAX_W = NG * 4 - 3;

// SrcArgs: what the layout's staging loop reads besides ImgArgs (image_stage.h; the contiguous RGB source is
// ImgArgs::img and takes NoSrc). Y: Src::YUV's and Src::YUV_TILES' Yuv<...>.
// Src::YUV_TILES: ImgArgs' h x w is the tile, the tap tables are the tile's, and the footprint they give is moved by
// the tile's origin into the frame before the column groups are laid out: the groups are the frame's (whatever the
// parity of the origin, a chroma pair lies under its luma as in the untiled launch), and the staging loops run on
// frame coordinates with batch element 0, so bilinear chroma clamps at the frame's edge, not at the tile's.
// One 256-thread workgroup per p x p patch: the patch's source footprint is staged in LDS, resampled horizontally
// into an fp32 LDS tile, then vertically by thread (u, v).
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
          // 4 luma bytes and the 2 chroma pairs under them; NV21 has V in a pair's first byte. Nearest chroma:
          // luma (r, c) takes chroma (r >> 1, c >> 1)
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
        } else if constexpr (S == Src::YUV || S == Src::YUV_TILES) {
          // the batch element: tiles are cut from one frame
          constexpr bool ONE = S == Src::YUV_TILES;
          if constexpr (Y::CHROMA == 1) stage_yuv_bilinear<Y>(n, ONE ? 0 : b, sy, sx, dst);
          else stage_yuv<Y>(n, ONE ? 0 : b, sy, sx, dst);
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
        // (of the dword that straddles an end of the image, the bytes inside, one by one)
        *reinterpret_cast<uint32_t*>(src + r * RS + d * 4) = load4(q, lo, hi);
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

// Every image kernel but the RGB one: the body for one source layout S with its arguments A (and, for the general YUV
// front end, its Yuv<...>).
template <Src S, class A, class Y = NoYuv>
__global__ __launch_bounds__(256) void image_patch_planes_k(ImgArgs a, A n) {
  image_patch_planes_body<S, A, Y>(a, n);
}

// The RGB kernel has no source arguments: an empty second parameter would still take a slot of the kernel's
// argument block and move the hidden arguments behind it.
__global__ __launch_bounds__(256) void image_patch_planes_u8(ImgArgs a) {
  image_patch_planes_body<Src::RGB>(a, NoSrc{});
}

template <class... A>
using Kernel = void (*)(ImgArgs, A...);

// The kernel of the general YUV front end for the arguments A and a Yuv<...>: over B tiles of one frame when A is
// Tiled.
template <class A, class Y>
constexpr Kernel<A> YUV_KERNEL = image_patch_planes_k<IS_TILED<A> ? Src::YUV_TILES : Src::YUV, A, Y>;

// The instantiations of the general YUV front end, by the arguments A the launch passes and a source s that yuv_args
// (and, for YuvHdrArgs, hdr_args) has checked. YuvArgs, nearest chroma: one per (layout, hsub, sample bytes), nine.
// YuvBilinearArgs, bilinear chroma: hsub is 1 and packed sources have one sample size, five. YuvHdrArgs, PQ and HLG
// through the tables: 16-bit samples, planar or semi-planar, 4:4:4 and subsampled with nearest chroma, subsampled
// with bilinear chroma, six. Tiled<A>: the same over B tiles of one frame.
template <class A>
Kernel<A> yuv_kernel(const NosYuvSrc& s) {
  if constexpr (std::is_base_of_v<YuvHdrArgs, A>) {
    switch ((s.layout == YUV_SEMI ? 3 : 0) + (s.chroma == 1 ? 2 : s.hsub)) {
      case 0: return YUV_KERNEL<A, Hdr<Yuv<YUV_PLANAR, 0, 2>>>;
      case 1: return YUV_KERNEL<A, Hdr<Yuv<YUV_PLANAR, 1, 2>>>;
      case 2: return YUV_KERNEL<A, Hdr<Yuv<YUV_PLANAR, 1, 2, 1>>>;
      case 3: return YUV_KERNEL<A, Hdr<Yuv<YUV_SEMI, 0, 2>>>;
      case 4: return YUV_KERNEL<A, Hdr<Yuv<YUV_SEMI, 1, 2>>>;
      default: return YUV_KERNEL<A, Hdr<Yuv<YUV_SEMI, 1, 2, 1>>>;
    }
  } else if constexpr (std::is_base_of_v<YuvBilinearArgs, A>) {
    switch (s.layout * 2 + (s.sample_bytes - 1)) {
      case 0: return YUV_KERNEL<A, Yuv<YUV_PLANAR, 1, 1, 1>>;
      case 1: return YUV_KERNEL<A, Yuv<YUV_PLANAR, 1, 2, 1>>;
      case 2: return YUV_KERNEL<A, Yuv<YUV_SEMI, 1, 1, 1>>;
      case 3: return YUV_KERNEL<A, Yuv<YUV_SEMI, 1, 2, 1>>;
      default: return YUV_KERNEL<A, Yuv<YUV_PACKED, 1, 1, 1>>;
    }
  } else {
    switch (s.layout * 4 + s.hsub * 2 + (s.sample_bytes - 1)) {
      case 0: return YUV_KERNEL<A, Yuv<YUV_PLANAR, 0, 1>>;
      case 1: return YUV_KERNEL<A, Yuv<YUV_PLANAR, 0, 2>>;
      case 2: return YUV_KERNEL<A, Yuv<YUV_PLANAR, 1, 1>>;
      case 3: return YUV_KERNEL<A, Yuv<YUV_PLANAR, 1, 2>>;
      case 4: return YUV_KERNEL<A, Yuv<YUV_SEMI, 0, 1>>;
      case 5: return YUV_KERNEL<A, Yuv<YUV_SEMI, 0, 2>>;
      case 6: return YUV_KERNEL<A, Yuv<YUV_SEMI, 1, 1>>;
      case 7: return YUV_KERNEL<A, Yuv<YUV_SEMI, 1, 2>>;
      default: return YUV_KERNEL<A, Yuv<YUV_PACKED, 1, 1>>;
    }
  }
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

// an image kernel on grid workgroups of 256 threads; what: the entry's name in the error a failed launch leaves
template <class... A>
int launch(Kernel<A...> kernel, int grid, void* stream, const char* what, const ImgArgs& k, const A&... n) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k, n...);
  return check(what);
}

// The arguments every image entry shares, in the order of the extern "C" signatures (nos_image_patch_planes_u8
// describes them).
struct Common {
  void* planes;
  float* pixels;
  const int* yidx;
  const float* ywt;
  const int* xidx;
  const float* xwt;
  int ytab, xtab, taps, max_fh, max_fw;
  const float *a, *b;
  int B, h, w, H, W, p, gh, gw, wgs;
  void* stream;
};

// what every image entry checks and fills (all but the source); grid: the workgroups to launch
int image_args(ImgArgs& k, int& grid, const Common& c) {
  if (!c.planes || !c.yidx || !c.ywt || !c.xidx || !c.xwt || !c.a || !c.b)
    return fail("image_patch_planes: null operand");
  if (c.B <= 0 || c.h <= 0 || c.w <= 0 || c.H <= 0 || c.W <= 0)
    return fail("image_patch_planes: B, h, w, H, W must be positive");
  if (c.p < 2 || c.p % 2 || c.p > PMAX) return fail("image_patch_planes: patch side must be even and at most 16");
  if (c.gh <= 0 || c.gw <= 0 || size_t(c.gh) * c.p > size_t(c.H) || size_t(c.gw) * c.p > size_t(c.W))
    return fail("image_patch_planes: whole patches inside the resized image (gh * p <= H, gw * p <= W)");
  if (c.taps != TAPS || c.ytab != c.H || c.xtab != c.W)
    return fail("image_patch_planes: tap tables must be [H][9] and [W][9]");
  if (c.max_fh <= 0 || c.max_fw <= 0 || c.max_fh > FMAX || c.max_fw > FMAX || c.max_fh > c.h || c.max_fw > c.w)
    return fail("image_patch_planes: a patch's source footprint exceeds 72 rows or columns (scale above 4)");
  k.planes = static_cast<__bf16*>(c.planes);
  k.pixels = c.pixels;
  k.yidx = c.yidx, k.ywt = c.ywt, k.xidx = c.xidx, k.xwt = c.xwt;
  for (int i = 0; i < 3; ++i) k.a[i] = c.a[i], k.b[i] = c.b[i];
  k.B = c.B, k.h = c.h, k.w = c.w, k.H = c.H, k.W = c.W, k.p = c.p, k.gh = c.gh, k.gw = c.gw;
  // with pixels every tile that covers H x W is computed; without, only the patch grid
  k.GH = c.pixels ? (c.H + c.p - 1) / c.p : c.gh;
  k.GW = c.pixels ? (c.W + c.p - 1) / c.p : c.gw;
  const size_t tiles = size_t(c.B) * k.GH * k.GW;
  if (tiles > size_t(1) << 30) return fail("image_patch_planes: too many patches");
  grid = int(c.wgs > 0 && size_t(c.wgs) < tiles ? size_t(c.wgs) : tiles);
  return 0;
}

PlaneArg plane_arg(const void* p, const void* lo, const void* hi, long long pitch, long long bs) {
  return PlaneArg{static_cast<const uint8_t*>(p), reinterpret_cast<uintptr_t>(lo), reinterpret_cast<uintptr_t>(hi), pitch,
                  bs};
}

// the plane q of B x rows x rowbytes (batch stride possibly negative) lies inside its storage [lo, hi)
bool inside(int B, const PlaneArg& q, long long rows, long long rowbytes) {
  const long long first = std::min(0LL, (B - 1) * q.bs),
                  last = std::max(0LL, (B - 1) * q.bs) + (rows - 1) * q.pitch + rowbytes;
  const intptr_t p = reinterpret_cast<intptr_t>(q.p);
  return q.lo && q.hi && p + first >= intptr_t(q.lo) && p + last <= intptr_t(q.hi);
}

bool stride_range(const PlaneArg& q) { return std::llabs(q.bs) <= (1LL << 40) && q.pitch <= (1LL << 30); }

// a colour table of codes of `depth` bits: coefficients that fit 24-bit multiplies, offsets that are codes
bool table_ok(const int* table, int depth) {
  for (int i = 0; i < 12; ++i)
    if (i < 9 ? std::abs(table[i]) >= (1 << 23) : (table[i] < 0 || table[i] >= (1 << depth))) return false;
  return true;
}

// every one of the B tiles of h x w at origins [B][2] (first row, first column) lies inside the frame
bool tiles_inside(const int* origins, int B, int h, int w, int frame_h, int frame_w) {
  for (int t = 0; t < B; ++t) {
    const long long y0 = origins[2 * t], x0 = origins[2 * t + 1];
    if (y0 < 0 || x0 < 0 || y0 + h > frame_h || x0 + w > frame_w) return false;
  }
  return true;
}

// A packed channel order ("rgb", "bgr", "rgba" or "bgra") as the colour offsets of n; the bytes of a pixel, or 0 for
// any other string.
int packed_order(const char* order, PackedArgs& n) {
  const std::string o(order);
  if (o != "rgb" && o != "bgr" && o != "rgba" && o != "bgra") return 0;
  n.r = o[0] == 'r' ? 0 : 2, n.g = 1, n.b = 2 - n.r;
  return int(o.size());
}

// both orders of the semi-planar entry: vu = 0 is NV12 (U, V), 1 is NV21 (V, U)
int patch_planes_semiplanar(const PlaneArg& y, const PlaneArg& uv, const int* table, const Common& c, int vu) {
  if (!y.p || !uv.p || !table) return fail("image_patch_planes: null operand");
  if (vu != 0 && vu != 1) return fail("image_patch_planes_nv12: the chroma order is 0 (U, V) or 1 (V, U)");
  ImgArgs k{};
  int grid = 0;
  if (const int rc = image_args(k, grid, c)) return rc;
  if (c.max_fw > GROUP_FMAX_W) return fail("image_patch_planes_nv12: a patch's source footprint exceeds 69 columns");
  const long long ch = (c.h + 1) / 2, cw2 = 2 * ((c.w + 1) / 2LL);
  if (y.pitch < c.w) return fail("image_patch_planes_nv12: the Y pitch is smaller than the width");
  if (uv.pitch < cw2) return fail("image_patch_planes_nv12: the UV pitch is smaller than 2 * ((w + 1) / 2)");
  if (!stride_range(y) || !stride_range(uv)) return fail("image_patch_planes_nv12: pitch or batch stride out of range");
  // the planes' first and one-past-last byte (a batch stride may be negative) inside the storage
  if (!inside(c.B, y, c.h, c.w) || !inside(c.B, uv, ch, cw2))
    return fail("image_patch_planes_nv12: a plane does not lie inside its storage bounds");
  if (!table_ok(table, 8))
    return fail("image_patch_planes_nv12: colour table: coefficients below 2^23 in size, offsets in 0..255");
  Nv12Args n{};
  n.y = y.p, n.uv = uv.p;
  n.ylo = y.lo, n.yhi = y.hi, n.uvlo = uv.lo, n.uvhi = uv.hi;
  n.ypitch = y.pitch, n.uvpitch = uv.pitch, n.ybs = y.bs, n.uvbs = uv.bs;
  for (int i = 0; i < 12; ++i) n.tab[i] = table[i];
  if (vu) return launch(image_patch_planes_k<Src::NV21, Nv12Args>, grid, c.stream, "image_patch_planes_nv21", k, n);
  return launch(image_patch_planes_k<Src::NV12, Nv12Args>, grid, c.stream, "image_patch_planes_nv12", k, n);
}

// The known combinations of a descriptor's layout, subsampling, sample format and order.
int yuv_format(const NosYuvSrc& s) {
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
  return 0;
}

// The planes of a descriptor whose format is known, holding sB frames of sh x sw, as pl[0..2]: every plane's first
// and last sample inside its storage [lo, hi). cw x ch: the size of a chroma plane in samples.
int yuv_planes(const NosYuvSrc& s, int sB, int sh, int sw, PlaneArg* pl, long long& cw, long long& ch) {
  const bool packed = s.layout == YUV_PACKED;
  // rows and row bytes of every plane
  const long long SB = s.sample_bytes;
  cw = (sw + (1LL << s.hsub) - 1) >> s.hsub, ch = (sh + (1LL << s.vsub) - 1) >> s.vsub;
  const int np = packed ? 1 : s.layout == YUV_SEMI ? 2 : 3;
  const long long rows[3] = {sh, ch, ch};
  const long long rowbytes[3] = {packed ? 4 * ((sw + 1LL) / 2) : sw * SB, s.layout == YUV_SEMI ? 2 * cw * SB : cw * SB,
                                 cw * SB};
  for (int i = 0; i < np; ++i) {
    const PlaneArg q = plane_arg(s.plane[i].p, s.plane[i].lo, s.plane[i].hi, s.plane[i].pitch, s.plane[i].bstride);
    if (!q.p) return fail("image_patch_planes: null operand");
    if (q.pitch < rowbytes[i]) return fail("image_patch_planes_yuv: a plane's pitch is smaller than its row's bytes");
    if (!stride_range(q)) return fail("image_patch_planes_yuv: pitch or batch stride out of range");
    if (SB == 2 && ((reinterpret_cast<uintptr_t>(q.p) | uintptr_t(q.pitch) | uintptr_t(q.bs)) & 1))
      return fail("image_patch_planes_yuv: 16-bit planes lie at an even address with an even pitch and batch stride");
    if (!inside(sB, q, rows[i], rowbytes[i]))
      return fail("image_patch_planes_yuv: a plane does not lie inside its storage bounds");
    pl[i] = q;
  }
  return 0;
}

// What the entries of the general YUV front end check and fill: every check of the descriptor and of the common
// arguments, then the kernel's arguments k and n and the workgroups to launch. sB x sh x sw: the batch and the size
// of the source the descriptor's planes hold — B x h x w itself, or the one frame that B tiles of h x w are cut from.
int yuv_args(const NosYuvSrc* src, ImgArgs& k, int& grid, YuvBilinearArgs& n, const Common& c, int sB, int sh, int sw) {
  if (!src) return fail("image_patch_planes: null operand");
  if (src->size != int(sizeof(NosYuvSrc)))
    return fail("image_patch_planes_yuv: descriptor size mismatch (NosYuvSrc of another build)");
  const NosYuvSrc& s = *src;
  if (const int rc = image_args(k, grid, c)) return rc;
  if (c.max_fw > GROUP_FMAX_W) return fail("image_patch_planes_yuv: a patch's source footprint exceeds 69 columns");
  if (const int rc = yuv_format(s)) return rc;
  if (s.chroma != 0 && s.chroma != 1)
    return fail("image_patch_planes_yuv: unknown chroma reconstruction (0 nearest, 1 bilinear)");
  if (s.siting < 0 || s.siting > 3)
    return fail("image_patch_planes_yuv: unknown chroma siting (bit 0 horizontally, bit 1 vertically co-sited)");
  if (s.chroma == 1 && s.hsub == 0)
    return fail("image_patch_planes_yuv: bilinear chroma takes a subsampled source (4:4:4 is launched as nearest)");
  long long cw = 0, ch = 0;
  if (const int rc = yuv_planes(s, sB, sh, sw, n.pl, cw, ch)) return rc;
  if (!table_ok(s.tab, s.depth))
    return fail("image_patch_planes_yuv: colour table: coefficients below 2^23 in size, offsets below 2^depth");
  for (int i = 0; i < 12; ++i) n.tab[i] = s.tab[i];
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

// The launch of the general YUV front end that takes the arguments A — n cut down to them — over the batch, or with
// a tile frame f over B tiles of one frame.
template <class A>
int yuv_launch_as(const NosYuvSrc& s, const ImgArgs& k, const YuvHdrArgs& n, const TileFrame* f, int grid,
                  void* stream, const char* what) {
  if (f) return launch(yuv_kernel<Tiled<A>>(s), grid, stream, what, k, Tiled<A>{A(n), *f});
  return launch(yuv_kernel<A>(s), grid, stream, what, k, A(n));
}

// The front end a checked source takes: HDR (the tables of n are filled), bilinear or nearest chroma.
int yuv_launch(const NosYuvSrc& s, bool hdr, const ImgArgs& k, const YuvHdrArgs& n, const TileFrame* f, int grid,
               void* stream, const char* what) {
  if (hdr) return yuv_launch_as<YuvHdrArgs>(s, k, n, f, grid, stream, what);
  if (s.chroma == 1) return yuv_launch_as<YuvBilinearArgs>(s, k, n, f, grid, stream, what);
  return yuv_launch_as<YuvArgs>(s, k, n, f, grid, stream, what);
}
// What both overlay entries check of the lists, the tables and the parameters, and fill of k.
int overlay_args(OverlayArgs& k, int h, int w, const int* count, const float* scores, const int* labels,
                 const float* boxes, const int* track_id, const int* track_hits, int N, const void* modes, int L,
                 const int* codes, int K, const int* font, int thickness, int scale, int min_hits) {
  if (!count || !scores || !labels || !boxes || !modes || !codes || !font) return fail("overlay: null operand");
  if ((track_id == nullptr) != (track_hits == nullptr)) return fail("overlay: track_id and track_hits go together");
  if (h <= 0 || w <= 0 || h > (1 << 15) || w > (1 << 15)) return fail("overlay: a frame of 1..32768 rows and columns");
  if (N <= 0 || N > OMAX) return fail("overlay: 0 < rows <= 1024");
  if (L <= 0 || K <= 0 || K > OVERLAY_MAX_K) return fail("overlay: labels > 0, 0 < colours <= 1024");
  if (thickness < 1 || thickness > OVERLAY_MAX_T || scale < 0 || scale > OVERLAY_MAX_S || min_hits < 1)
    return fail("overlay: 1 <= thickness <= 2^20, 0 <= scale <= 1024, min_hits >= 1");
  k = OverlayArgs{count, scores, labels, boxes, track_id, track_hits, static_cast<const uint8_t*>(modes), codes, font,
                  N, L, K, thickness, scale, min_hits, h, w};
  return 0;
}

// overlay_k on one workgroup per tile of the h x w frame
template <class Dst>
int overlay_launch(const OverlayArgs& k, const Dst& dst, void* stream, const char* what) {
  const int grid = ((k.h + OTH - 1) / OTH) * ((k.w + OTW - 1) / OTW);
  hipLaunchKernelGGL(overlay_k<Dst>, dim3(grid), dim3(OT), 0, reinterpret_cast<hipStream_t>(stream), k, dst);
  return check(what);
}
}  // namespace

extern "C" {

const char* nos_image_last_error() { return g_err.c_str(); }

int nos_image_taps() { return TAPS; }
int nos_image_max_footprint() { return FMAX; }
int nos_image_max_patch() { return PMAX; }

// the widest footprint of the layouts that stage column groups: one constant, an entry per family of layouts
int nos_image_nv12_max_footprint() { return GROUP_FMAX_W; }
int nos_image_yuv420p_max_footprint() { return GROUP_FMAX_W; }
int nos_image_packed_max_footprint() { return GROUP_FMAX_W; }
int nos_image_yuv_max_footprint() { return GROUP_FMAX_W; }

// img [B][h][w][3] uint8 -> planes [3][B*gh*gw][3*p*p] bf16 (and pixels [B][3][H][W] fp32 when
// non-null). yidx [2][H] / xidx [2][W] (first source index, tap count) and ywt [H][taps] / xwt
// [W][taps] are device tables; ytab / xtab are their row counts, max_fh / max_fw the largest source
// footprint of one patch row / column of those tables (the host built them, so it knows). a, b:
// host arrays of the three per-channel affine constants. wgs: workgroups (0 = one per tile).
int nos_image_patch_planes_u8(const void* img, void* planes, float* pixels, const int* yidx, const float* ywt,
                              const int* xidx, const float* xwt, int ytab, int xtab, int taps, int max_fh, int max_fw,
                              const float* a, const float* b, int B, int h, int w, int H, int W, int p, int gh, int gw,
                              int wgs, void* stream) {
  const Common c{planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b, B, h, w, H, W, p, gh, gw,
                 wgs, stream};
  if (!img) return fail("image_patch_planes: null operand");
  ImgArgs k{};
  int grid = 0;
  if (const int rc = image_args(k, grid, c)) return rc;
  k.img = static_cast<const uint8_t*>(img);
  return launch(image_patch_planes_u8, grid, stream, "image_patch_planes_u8", k);
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
  const Common c{planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b, B, h, w, H, W, p, gh, gw,
                 wgs, stream};
  return patch_planes_semiplanar(plane_arg(y, y_lo, y_hi, y_pitch, y_bstride),
                                 plane_arg(uv, uv_lo, uv_hi, uv_pitch, uv_bstride), table, c, 0);
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
  const Common c{planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b, B, h, w, H, W, p, gh, gw,
                 wgs, stream};
  return patch_planes_semiplanar(plane_arg(y, y_lo, y_hi, y_pitch, y_bstride),
                                 plane_arg(uv, uv_lo, uv_hi, uv_pitch, uv_bstride), table, c, vu);
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
  const Common c{planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b, B, h, w, H, W, p, gh, gw,
                 wgs, stream};
  if (!y || !u || !v || !table) return fail("image_patch_planes: null operand");
  ImgArgs k{};
  int grid = 0;
  if (const int rc = image_args(k, grid, c)) return rc;
  if (max_fw > GROUP_FMAX_W) return fail("image_patch_planes_yuv420p: a patch's source footprint exceeds 69 columns");
  const long long ch = (h + 1) / 2, cw = (w + 1) / 2;
  PlanarArgs n{};
  n.y = plane_arg(y, y_lo, y_hi, y_pitch, y_bstride);
  n.u = plane_arg(u, u_lo, u_hi, u_pitch, u_bstride);
  n.v = plane_arg(v, v_lo, v_hi, v_pitch, v_bstride);
  if (y_pitch < w) return fail("image_patch_planes_yuv420p: the Y pitch is smaller than the width");
  if (u_pitch < cw) return fail("image_patch_planes_yuv420p: the U pitch is smaller than (w + 1) / 2");
  if (v_pitch < cw) return fail("image_patch_planes_yuv420p: the V pitch is smaller than (w + 1) / 2");
  if (!stride_range(n.y) || !stride_range(n.u) || !stride_range(n.v))
    return fail("image_patch_planes_yuv420p: pitch or batch stride out of range");
  if (!inside(B, n.y, h, w) || !inside(B, n.u, ch, cw) || !inside(B, n.v, ch, cw))
    return fail("image_patch_planes_yuv420p: a plane does not lie inside its storage bounds");
  if (!table_ok(table, 8))
    return fail("image_patch_planes_yuv420p: colour table: coefficients below 2^23 in size, offsets in 0..255");
  for (int i = 0; i < 12; ++i) n.tab[i] = table[i];
  return launch(image_patch_planes_k<Src::YUV420P, PlanarArgs>, grid, stream, "image_patch_planes_yuv420p", k, n);
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
  const Common c{planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b, B, h, w, H, W, p, gh, gw,
                 wgs, stream};
  if (!img || !order) return fail("image_patch_planes: null operand");
  PackedArgs n{};
  const int C = packed_order(order, n);
  if (!C) return fail("image_patch_planes_packed: unknown channel order (rgb, bgr, rgba or bgra)");
  ImgArgs k{};
  int grid = 0;
  if (const int rc = image_args(k, grid, c)) return rc;
  if (max_fw > GROUP_FMAX_W) return fail("image_patch_planes_packed: a patch's source footprint exceeds 69 columns");
  n.s = plane_arg(img, lo, hi, pitch, bstride);
  if (pitch < (long long)w * C) return fail("image_patch_planes_packed: the row pitch is smaller than a row's bytes");
  if (!stride_range(n.s)) return fail("image_patch_planes_packed: pitch or batch stride out of range");
  if (!inside(B, n.s, h, (long long)w * C))
    return fail("image_patch_planes_packed: the image does not lie inside its storage bounds");
  if (C == 4) return launch(image_patch_planes_k<Src::PACKED4, PackedArgs>, grid, stream, "image_patch_planes_packed", k, n);
  return launch(image_patch_planes_k<Src::PACKED3, PackedArgs>, grid, stream, "image_patch_planes_packed", k, n);
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
  const Common c{planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b, B, h, w, H, W, p, gh, gw,
                 wgs, stream};
  if (!img || !order) return fail("image_patch_planes: null operand");
  if (!origins || !table) return fail("image_patch_planes_tiles: null origin table");
  PackedTileArgs n{};
  const int C = packed_order(order, n);
  if (!C) return fail("image_patch_planes_tiles: unknown channel order (rgb, bgr, rgba or bgra)");
  ImgArgs k{};
  int grid = 0;
  if (const int rc = image_args(k, grid, c)) return rc;
  if (max_fw > GROUP_FMAX_W) return fail("image_patch_planes_tiles: a patch's source footprint exceeds 69 columns");
  if (frame_h <= 0 || frame_w <= 0) return fail("image_patch_planes_tiles: the frame's sizes must be positive");
  n.s = plane_arg(img, lo, hi, pitch, 0);
  n.origin = table;
  if (pitch < (long long)frame_w * C) return fail("image_patch_planes_tiles: the row pitch is smaller than a row's bytes");
  if (!stride_range(n.s)) return fail("image_patch_planes_tiles: pitch out of range");
  if (!inside(1, n.s, frame_h, (long long)frame_w * C))
    return fail("image_patch_planes_tiles: the frame does not lie inside its storage bounds");
  if (!tiles_inside(origins, B, h, w, frame_h, frame_w))
    return fail("image_patch_planes_tiles: a tile does not lie inside the frame");
  if (C == 4)
    return launch(image_patch_planes_k<Src::TILES4, PackedTileArgs>, grid, stream, "image_patch_planes_tiles", k, n);
  return launch(image_patch_planes_k<Src::TILES3, PackedTileArgs>, grid, stream, "image_patch_planes_tiles", k, n);
}

// The same from any YUV surface NosYuvSrc (image_yuv.h) describes: planar, semi-planar or packed 4:2:2; 4:2:0,
// 4:2:2 or 4:4:4; 8-bit samples or 10 / 12-bit codes in little-endian 16-bit words (in the high or the low bits;
// the other bits are ignored, not required to be zero). Nothing is launched unless every check passes.
int nos_image_patch_planes_yuv(const NosYuvSrc* src, void* planes, float* pixels, const int* yidx, const float* ywt,
                               const int* xidx, const float* xwt, int ytab, int xtab, int taps, int max_fh, int max_fw,
                               const float* a, const float* b, int B, int h, int w, int H, int W, int p, int gh, int gw,
                               int wgs, void* stream) {
  const Common c{planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b, B, h, w, H, W, p, gh, gw,
                 wgs, stream};
  ImgArgs k{};
  int grid = 0;
  YuvHdrArgs n{};
  if (const int rc = yuv_args(src, k, grid, n, c, B, h, w)) return rc;
  return yuv_launch(*src, false, k, n, nullptr, grid, stream, "image_patch_planes_yuv");
}

// The same of a source whose codes are PQ or HLG, through the tables NosYuvHdr (image_yuv.h) points to: 10 / 12-bit
// codes in 16-bit words, planar or semi-planar, nearest or bilinear chroma. Every check of nos_image_patch_planes_yuv,
// then those of the tables; nothing is launched unless all pass.
int nos_image_patch_planes_yuv_hdr(const NosYuvSrc* src, const NosYuvHdr* hdr, void* planes, float* pixels,
                                   const int* yidx, const float* ywt, const int* xidx, const float* xwt, int ytab,
                                   int xtab, int taps, int max_fh, int max_fw, const float* a, const float* b, int B,
                                   int h, int w, int H, int W, int p, int gh, int gw, int wgs, void* stream) {
  const Common c{planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b, B, h, w, H, W, p, gh, gw,
                 wgs, stream};
  if (!hdr) return fail("image_patch_planes: null operand");
  if (hdr->size != int(sizeof(NosYuvHdr)))
    return fail("image_patch_planes_yuv_hdr: table descriptor size mismatch (NosYuvHdr of another build)");
  ImgArgs k{};
  int grid = 0;
  YuvHdrArgs n{};
  if (const int rc = yuv_args(src, k, grid, n, c, B, h, w)) return rc;
  if (const int rc = hdr_args(*src, *hdr, n)) return rc;
  return yuv_launch(*src, true, k, n, nullptr, grid, stream, "image_patch_planes_yuv_hdr");
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
  const Common c{planes, pixels, yidx, ywt, xidx, xwt, ytab, xtab, taps, max_fh, max_fw, a, b, B, h, w, H, W, p, gh, gw,
                 wgs, stream};
  if (!origins || !table) return fail("image_patch_planes_yuv_tiles: null origin table");
  if (frames != 1) return fail("image_patch_planes_yuv_tiles: tiles are cut from one frame (a source batch of 1)");
  if (frame_h <= 0 || frame_w <= 0) return fail("image_patch_planes_yuv_tiles: the frame's sizes must be positive");
  if (hdr && hdr->size != int(sizeof(NosYuvHdr)))
    return fail("image_patch_planes_yuv_hdr: table descriptor size mismatch (NosYuvHdr of another build)");
  ImgArgs k{};
  int grid = 0;
  YuvHdrArgs n{};
  if (const int rc = yuv_args(src, k, grid, n, c, 1, frame_h, frame_w)) return rc;
  if (hdr)
    if (const int rc = hdr_args(*src, *hdr, n)) return rc;
  if (!tiles_inside(origins, B, h, w, frame_h, frame_w))
    return fail("image_patch_planes_yuv_tiles: a tile does not lie inside the frame");
  const TileFrame f{table, frame_h, frame_w};
  return yuv_launch(*src, hdr != nullptr, k, n, &f, grid, stream, "image_patch_planes_yuv_tiles");
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

// One frame's detections associated with a tracker's state, which is updated in place (track_update_f32): count [1]
// int32, scores [N] fp32, labels [N] int32, boxes [N][4] fp32 (corners), as the two entries above write them; the state
// t_boxes / t_vel [T][4] fp32, t_labels / t_ids / t_hits / t_misses [T] int32, next_id [1], dropped [1] int32; motion: 0
// no prediction, 1 constant velocity with velocity_gain in [0, 1] -> track_id [N], track_hits [N] int32 by input row
int nos_track_update_f32(const int* count, const float* scores, const int* labels, const float* boxes, int N,
                         float* t_boxes, float* t_vel, int* t_labels, int* t_ids, int* t_hits, int* t_misses,
                         int* next_id, int* dropped, int T, float match_threshold, int max_age, float birth_threshold,
                         int motion, float velocity_gain, int* track_id, int* track_hits, void* stream) {
  if (!count || !scores || !labels || !boxes || !t_boxes || !t_vel || !t_labels || !t_ids || !t_hits || !t_misses ||
      !next_id || !dropped || !track_id || !track_hits)
    return fail("track_update: null operand");
  if (N <= 0 || N > MMAX || T <= 0 || T > TMAX) return fail("track_update: 0 < rows <= 1024, 0 < slots <= 1024");
  if (motion != 0 && motion != 1) return fail("track_update: the motion is 0 (none) or 1 (constant)");
  if (!(match_threshold >= 0.f) || max_age < 0 || !(velocity_gain >= 0.f && velocity_gain <= 1.f))
    return fail("track_update: match_threshold >= 0, max_age >= 0, 0 <= velocity_gain <= 1");
  hipLaunchKernelGGL(track_update_f32, dim3(1), dim3(DT), 0, reinterpret_cast<hipStream_t>(stream), count, scores,
                     labels, boxes, N, t_boxes, t_vel, t_labels, t_ids, t_hits, t_misses, next_id, dropped, T,
                     match_threshold, max_age, birth_threshold, motion, velocity_gain, track_id, track_hits);
  return check("track_update_f32");
}

int nos_overlay_tile_rows() { return OTH; }
int nos_overlay_tile_columns() { return OTW; }

// One frame's detections painted into packed pixels img [h][w][C] (order, pitch and [lo, hi) as in
// nos_image_patch_planes_packed; the fourth byte of a pixel is never written): count [1] int32, scores [N] fp32, labels
// [N] int32, boxes [N][4] fp32 as the entries above write them, track_id / track_hits [N] int32 as nos_track_update_f32
// does or both null; modes [L] uint8, codes [2 K + 1][3] int32 and font [10][7] int32 are device tables
// (image_overlay.h). Nothing is launched unless every check passes, the first and last byte of the image inside
// [lo, hi) among them; the kernel stores nothing outside pixels (y, x) with y < h and x < w.
int nos_overlay_packed(void* img, const void* lo, const void* hi, long long pitch, const char* order, int h, int w,
                       const int* count, const float* scores, const int* labels, const float* boxes,
                       const int* track_id, const int* track_hits, int N, const void* modes, int L, const int* codes,
                       int K, const int* font, int thickness, int scale, int min_hits, void* stream) {
  if (!img || !order) return fail("overlay: null operand");
  PackedArgs o{};
  const int C = packed_order(order, o);
  if (!C) return fail("overlay_packed: unknown channel order (rgb, bgr, rgba or bgra)");
  OverlayArgs k{};
  if (const int rc = overlay_args(k, h, w, count, scores, labels, boxes, track_id, track_hits, N, modes, L, codes, K,
                                  font, thickness, scale, min_hits))
    return rc;
  const PackedDst dst{plane_arg(img, lo, hi, pitch, 0), C, o.r};
  if (pitch < (long long)w * C) return fail("overlay_packed: the row pitch is smaller than a row's bytes");
  if (!stride_range(dst.s)) return fail("overlay_packed: pitch out of range");
  if (!inside(1, dst.s, h, (long long)w * C)) return fail("overlay_packed: the image does not lie inside its storage bounds");
  return overlay_launch(k, dst, stream, "overlay_packed");
}

// The same into the one h x w frame of any YUV surface NosYuvSrc describes (tab, chroma and siting are not read): the
// luma sample of every painted pixel, and a chroma sample where its top-left luma pixel is painted; 16-bit samples as
// whole words, code << shift. codes holds Y, U, V codes of the surface's depth. Every check of the descriptor that
// nos_image_patch_planes_yuv makes of its planes, the first and last sample of each inside its [lo, hi).
int nos_overlay_yuv(const NosYuvSrc* dst, int h, int w, const int* count, const float* scores, const int* labels,
                    const float* boxes, const int* track_id, const int* track_hits, int N, const void* modes, int L,
                    const int* codes, int K, const int* font, int thickness, int scale, int min_hits, void* stream) {
  if (!dst) return fail("overlay: null operand");
  if (dst->size != int(sizeof(NosYuvSrc))) return fail("overlay_yuv: descriptor size mismatch (NosYuvSrc of another build)");
  OverlayArgs k{};
  if (const int rc = overlay_args(k, h, w, count, scores, labels, boxes, track_id, track_hits, N, modes, L, codes, K,
                                  font, thickness, scale, min_hits))
    return rc;
  YuvDst d{};
  long long cw = 0, ch = 0;
  if (yuv_format(*dst) || yuv_planes(*dst, 1, h, w, d.pl, cw, ch)) {
    g_err = "overlay_yuv: the surface: " + g_err;
    return -1;
  }
  d.layout = dst->layout, d.hsub = dst->hsub, d.vsub = dst->vsub, d.sb = dst->sample_bytes, d.shift = dst->shift;
  d.order = dst->order;
  return overlay_launch(k, d, stream, "overlay_yuv");
}

}  // extern "C"
