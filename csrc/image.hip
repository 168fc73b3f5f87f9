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
//  * Pixelating (image_mosaic.h): mosaic_k, the cells a selected detection touches replaced by their mean, in place —
//    the one kernel here that reads a surface and writes it.
//  * Blurring (image_blur.h): blur_snapshot_k and blur_k, the detections of selected labels blurred in place through a
//    shadow copy of what a blur can read: two launches, no traffic between workgroups.
//  * Cutting (image_chips.h): chips_k, the detections of selected labels cut out of any source the patch kernel reads and
//    resampled to one size as RGB bytes — the one kernel here that reads a surface and writes a new tensor.
//  * Resizing (image_scale.h): rescale_k, a frame resized into a second surface of the same layout by the chips' exact
//    area average, plane by plane — the one kernel here that writes a frame it did not read.
//  * Converting (image_convert.h): convert_k, a frame of any source the chips read written into a second surface of any
//    SDR layout, depth, subsampling and order at any size — the chips' read side, the forward colour rule, rescale_k's
//    whole storage units.
//  * Appearance (image_features.h): chip_features_k, feature_overlap_k and track_features_k — a colour descriptor per
//    chip, its intersection with every track's, and the descriptor a track keeps — around track_update_app_f32
//    (image_track.h), the tracker gated and re-identified by them.
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
#include "image_mosaic.h"
#include "image_blur.h"
#include "image_scale.h"
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
}  // namespace

#include "image_chips.h"  // behind the source tags: chips_k is instantiated by them
#include "image_convert.h"
#include "image_features.h"

namespace {

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

// The instantiations of the general YUV front end, by the arguments A the launch passes and a source s that yuv_source
// (and, for YuvHdrArgs, hdr_args) has checked: f is called with the source's Yuv<...> tag and says what is
// instantiated by it. YuvArgs, nearest chroma: one per (layout, hsub, sample bytes), nine. YuvBilinearArgs, bilinear
// chroma: hsub is 1 and packed sources have one sample size, five. YuvHdrArgs, PQ and HLG through the tables: 16-bit
// samples, planar or semi-planar, 4:4:4 and subsampled with nearest chroma, subsampled with bilinear chroma, six.
// The one table of the patch kernel (yuv_kernel) and of the chips (chips_yuv_kernel).
template <class A, class F>
auto yuv_dispatch(const NosYuvSrc& s, F f) {
  if constexpr (std::is_base_of_v<YuvHdrArgs, A>) {
    switch ((s.layout == YUV_SEMI ? 3 : 0) + (s.chroma == 1 ? 2 : s.hsub)) {
      case 0: return f(Hdr<Yuv<YUV_PLANAR, 0, 2>>{});
      case 1: return f(Hdr<Yuv<YUV_PLANAR, 1, 2>>{});
      case 2: return f(Hdr<Yuv<YUV_PLANAR, 1, 2, 1>>{});
      case 3: return f(Hdr<Yuv<YUV_SEMI, 0, 2>>{});
      case 4: return f(Hdr<Yuv<YUV_SEMI, 1, 2>>{});
      default: return f(Hdr<Yuv<YUV_SEMI, 1, 2, 1>>{});
    }
  } else if constexpr (std::is_base_of_v<YuvBilinearArgs, A>) {
    switch (s.layout * 2 + (s.sample_bytes - 1)) {
      case 0: return f(Yuv<YUV_PLANAR, 1, 1, 1>{});
      case 1: return f(Yuv<YUV_PLANAR, 1, 2, 1>{});
      case 2: return f(Yuv<YUV_SEMI, 1, 1, 1>{});
      case 3: return f(Yuv<YUV_SEMI, 1, 2, 1>{});
      default: return f(Yuv<YUV_PACKED, 1, 1, 1>{});
    }
  } else {
    switch (s.layout * 4 + s.hsub * 2 + (s.sample_bytes - 1)) {
      case 0: return f(Yuv<YUV_PLANAR, 0, 1>{});
      case 1: return f(Yuv<YUV_PLANAR, 0, 2>{});
      case 2: return f(Yuv<YUV_PLANAR, 1, 1>{});
      case 3: return f(Yuv<YUV_PLANAR, 1, 2>{});
      case 4: return f(Yuv<YUV_SEMI, 0, 1>{});
      case 5: return f(Yuv<YUV_SEMI, 0, 2>{});
      case 6: return f(Yuv<YUV_SEMI, 1, 1>{});
      case 7: return f(Yuv<YUV_SEMI, 1, 2>{});
      default: return f(Yuv<YUV_PACKED, 1, 1>{});
    }
  }
}

// The patch kernel of a checked source: over B tiles of one frame when A is Tiled.
template <class A>
Kernel<A> yuv_kernel(const NosYuvSrc& s) {
  return yuv_dispatch<A>(s, [](auto y) -> Kernel<A> { return YUV_KERNEL<A, decltype(y)>; });
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

// a refusal of an entry that shares its checks with another: "<who><msg>"
int fail(const char* who, const std::string& msg) {
  g_err = who + msg;
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

// The storage planes of one frame: how many there are, the rows and the row bytes of each, and for a YUV surface
// cw x ch, the size of a chroma plane in samples.
struct PlaneSizes {
  int np;
  long long rows[3], rowbytes[3], cw, ch;
};

// Those of a YUV surface of h x w whose format is known.
PlaneSizes yuv_sizes(const NosYuvSrc& s, int h, int w) {
  const bool packed = s.layout == YUV_PACKED, semi = s.layout == YUV_SEMI;
  const long long SB = s.sample_bytes;
  PlaneSizes z{packed ? 1 : semi ? 2 : 3};
  z.cw = (w + (1LL << s.hsub) - 1) >> s.hsub, z.ch = (h + (1LL << s.vsub) - 1) >> s.vsub;
  z.rows[0] = h, z.rows[1] = z.rows[2] = z.ch;
  z.rowbytes[0] = packed ? 4 * ((w + 1LL) / 2) : w * SB;       // a macropixel of two pixels is four bytes
  z.rowbytes[1] = semi ? 2 * z.cw * SB : z.cw * SB, z.rowbytes[2] = z.cw * SB;
  return z;
}

// The planes of a descriptor whose format is known, holding sB frames of sh x sw, as pl[0..2]: every plane's first
// and last sample inside its storage [lo, hi). z: yuv_sizes of sh x sw.
int yuv_planes(const NosYuvSrc& s, int sB, const PlaneSizes& z, PlaneArg* pl) {
  for (int i = 0; i < z.np; ++i) {
    const PlaneArg q = plane_arg(s.plane[i].p, s.plane[i].lo, s.plane[i].hi, s.plane[i].pitch, s.plane[i].bstride);
    if (!q.p) return fail("image_patch_planes: null operand");
    if (q.pitch < z.rowbytes[i]) return fail("image_patch_planes_yuv: a plane's pitch is smaller than its row's bytes");
    if (!stride_range(q)) return fail("image_patch_planes_yuv: pitch or batch stride out of range");
    if (s.sample_bytes == 2 && ((reinterpret_cast<uintptr_t>(q.p) | uintptr_t(q.pitch) | uintptr_t(q.bs)) & 1))
      return fail("image_patch_planes_yuv: 16-bit planes lie at an even address with an even pitch and batch stride");
    if (!inside(sB, q, z.rows[i], z.rowbytes[i]))
      return fail("image_patch_planes_yuv: a plane does not lie inside its storage bounds");
    pl[i] = q;
  }
  return 0;
}

// What every entry that reads a YUV source checks of a descriptor of the right size, and fills of n: the format, the
// chroma reconstruction, the planes of sB frames of sh x sw inside their storage, the colour table.
int yuv_source(const NosYuvSrc& s, YuvBilinearArgs& n, int sB, int sh, int sw) {
  if (const int rc = yuv_format(s)) return rc;
  if (s.chroma != 0 && s.chroma != 1)
    return fail("image_patch_planes_yuv: unknown chroma reconstruction (0 nearest, 1 bilinear)");
  if (s.siting < 0 || s.siting > 3)
    return fail("image_patch_planes_yuv: unknown chroma siting (bit 0 horizontally, bit 1 vertically co-sited)");
  if (s.chroma == 1 && s.hsub == 0)
    return fail("image_patch_planes_yuv: bilinear chroma takes a subsampled source (4:4:4 is launched as nearest)");
  const PlaneSizes z = yuv_sizes(s, sh, sw);
  if (const int rc = yuv_planes(s, sB, z, n.pl)) return rc;
  if (!table_ok(s.tab, s.depth))
    return fail("image_patch_planes_yuv: colour table: coefficients below 2^23 in size, offsets below 2^depth");
  for (int i = 0; i < 12; ++i) n.tab[i] = s.tab[i];
  n.vsub = s.vsub, n.depth = s.depth, n.shift = s.shift, n.mask = (1 << s.depth) - 1, n.order = s.order;
  // co-sited: (4, 0) of C[i], C[i] at an even position, held as (0, 4) of C[i - 1], C[i], and (2, 2) at an odd one;
  // centred: (1, 3) and (3, 1)
  n.cw = int(z.cw), n.ch = int(z.ch);
  static const int cosited[4] = {0, 4, 2, 2}, centred[4] = {1, 3, 3, 1};
  for (int i = 0; i < 4; ++i)
    n.wx[i] = (s.siting & 1 ? cosited : centred)[i], n.wy[i] = (s.siting & 2 ? cosited : centred)[i];
  return 0;
}

// What the entries of the general YUV front end check and fill: every check of the descriptor and of the common
// arguments, then the kernel's arguments k and n and the workgroups to launch. sB x sh x sw: the batch and the size
// of the source the descriptor's planes hold — B x h x w itself, or the one frame that B tiles of h x w are cut from.
int yuv_args(const NosYuvSrc* src, ImgArgs& k, int& grid, YuvBilinearArgs& n, const Common& c, int sB, int sh, int sw) {
  if (!src) return fail("image_patch_planes: null operand");
  if (src->size != int(sizeof(NosYuvSrc)))
    return fail("image_patch_planes_yuv: descriptor size mismatch (NosYuvSrc of another build)");
  if (const int rc = image_args(k, grid, c)) return rc;
  if (c.max_fw > GROUP_FMAX_W) return fail("image_patch_planes_yuv: a patch's source footprint exceeds 69 columns");
  return yuv_source(*src, n, sB, sh, sw);
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
// One frame's lists as the effect entries take them: N rows, track_id and track_hits both null or both given, the [L]
// table of labels (modes or select, uint8), and min_hits.
struct Lists {
  const int* count;
  const float* scores;
  const int* labels;
  const float* boxes;
  const int *track_id, *track_hits;
  const void* table;
  int N, L, min_hits;
};

// What every effect entry checks of one frame's lists and of the frame's size.
int list_args(const char* who, int h, int w, const Lists& l) {
  const char* msg = nullptr;
  if (!l.count || !l.scores || !l.labels || !l.boxes || !l.table) msg = ": null operand";
  else if ((l.track_id == nullptr) != (l.track_hits == nullptr)) msg = ": track_id and track_hits go together";
  else if (h <= 0 || w <= 0 || h > (1 << 15) || w > (1 << 15)) msg = ": a frame of 1..32768 rows and columns";
  else if (l.N <= 0 || l.N > OMAX) msg = ": 0 < rows <= 1024";
  else if (l.L <= 0 || l.min_hits < 1) msg = ": labels > 0, min_hits >= 1";
  return msg ? fail(who, msg) : 0;
}

// What both overlay entries check of the lists, the tables and the parameters, and fill of k.
int overlay_args(OverlayArgs& k, int h, int w, const Lists& l, const int* codes, int K, const int* font, int thickness,
                 int scale) {
  if (!codes || !font) return fail("overlay: null operand");
  if (const int rc = list_args("overlay", h, w, l)) return rc;
  if (K <= 0 || K > OVERLAY_MAX_K) return fail("overlay: 0 < colours <= 1024");
  if (thickness < 1 || thickness > OVERLAY_MAX_T || scale < 0 || scale > OVERLAY_MAX_S)
    return fail("overlay: 1 <= thickness <= 2^20, 0 <= scale <= 1024");
  k = OverlayArgs{l.count, l.scores, l.labels, l.boxes, l.track_id, l.track_hits, static_cast<const uint8_t*>(l.table),
                  codes, font, l.N, l.L, K, thickness, scale, l.min_hits, h, w};
  return 0;
}

// What the selecting effects (who: mosaic, blur, chips) check of the lists, and the MosaicArgs they share: no cell, the
// mask of a byte (a YUV entry fills in the surface's).
int select_args(const char* who, MosaicArgs& m, int h, int w, const Lists& l) {
  if (const int rc = list_args(who, h, w, l)) return rc;
  m = MosaicArgs{l.count, l.scores, l.labels, l.boxes, l.track_id, l.track_hits, static_cast<const uint8_t*>(l.table),
                 l.N, l.L, l.min_hits, h, w, 0, 255};
  return 0;
}

// What both mosaic entries check and fill of k.
int mosaic_args(MosaicArgs& k, int h, int w, const Lists& l, int cell) {
  if (const int rc = select_args("mosaic", k, h, w, l)) return rc;
  if (cell < MOSAIC_MIN_CELL || cell > MTILE || (cell & (cell - 1))) return fail("mosaic: a cell of 4, 8, 16, 32 or 64 pixels");
  k.cell = cell;
  return 0;
}

// overlay_k on one workgroup per tile of the h x w frame
template <class Dst>
int overlay_launch(const OverlayArgs& k, const Dst& dst, void* stream, const char* what) {
  const int grid = ((k.h + OTH - 1) / OTH) * ((k.w + OTW - 1) / OTW);
  hipLaunchKernelGGL(overlay_k<Dst>, dim3(grid), dim3(OT), 0, reinterpret_cast<hipStream_t>(stream), k, dst);
  return check(what);
}

// mosaic_k on one workgroup per tile of the h x w frame
template <class Dst>
int mosaic_launch(const MosaicArgs& k, const Dst& dst, void* stream, const char* what) {
  const int grid = ((k.h + MTILE - 1) / MTILE) * ((k.w + MTILE - 1) / MTILE);
  hipLaunchKernelGGL(mosaic_k<Dst>, dim3(grid), dim3(MT), 0, reinterpret_cast<hipStream_t>(stream), k, dst);
  return check(what);
}

// The checks both packed entries (who: overlay_packed, mosaic_packed) make of the image and its order; fills dst.
int packed_dst(const char* who, PackedDst& dst, void* img, const void* lo, const void* hi, long long pitch,
               const char* order, int h, int w) {
  PackedArgs o{};
  const int C = packed_order(order, o);
  if (!C) return fail(who, ": unknown channel order (rgb, bgr, rgba or bgra)");
  dst = PackedDst{plane_arg(img, lo, hi, pitch, 0), C, o.r};
  if (pitch < (long long)w * C) return fail(who, ": the row pitch is smaller than a row's bytes");
  if (!stride_range(dst.s)) return fail(who, ": pitch out of range");
  if (!inside(1, dst.s, h, (long long)w * C)) return fail(who, ": the image does not lie inside its storage bounds");
  return 0;
}

// What the YUV effect entries open with: the descriptor is there ("<effect>: ...") and of this build ("<entry>: ...").
int yuv_open(const char* effect, const char* entry, const NosYuvSrc* s) {
  if (!s) return fail(effect, ": null operand");
  if (s->size != int(sizeof(NosYuvSrc))) return fail(entry, ": descriptor size mismatch (NosYuvSrc of another build)");
  return 0;
}

// The checks the YUV effect entries (who: overlay_yuv, ...) make of the descriptor's format and planes; fills d.
int yuv_dst(const char* who, YuvDst& d, const NosYuvSrc& s, int h, int w) {
  if (yuv_format(s) || yuv_planes(s, 1, yuv_sizes(s, h, w), d.pl)) return fail(who, ": the surface: " + g_err);
  d.layout = s.layout, d.hsub = s.hsub, d.vsub = s.vsub, d.sb = s.sample_bytes, d.shift = s.shift, d.order = s.order;
  return 0;
}

// The shadow of z.np planes (image_blur.h): plane i lies behind plane i - 1 at its own pitch, at its own address modulo
// 4. Returns the bytes a shadow needs at most; with a shadow, fills out[i].p (the rest of out[i] is pl[i]'s).
long long blur_shadow(const PlaneArg* pl, const PlaneSizes& z, void* shadow, PlaneArg* out) {
  long long at = 0;
  for (int i = 0; i < z.np; ++i) {
    if (shadow) {
      uint8_t* q = static_cast<uint8_t*>(shadow) + at;
      q += (reinterpret_cast<uintptr_t>(pl[i].p) - reinterpret_cast<uintptr_t>(q)) & 3;
      out[i] = pl[i], out[i].p = q;
    }
    at += (z.rows[i] - 1) * pl[i].pitch + z.rowbytes[i] + 4;
  }
  return at;
}

// The rows of a band (image_blur.h) at `radius` with partials of pb bytes: 64 where the codes and partials of 64 rows
// fit BLUR_BAND_LDS, else 32.
constexpr int BLUR_BAND_LDS = 48 << 10;
int blur_band(int radius, int pb) { return blur_lds(BTILE, radius, radius, pb) <= BLUR_BAND_LDS ? BTILE : BTILE / 2; }

// What both blur entries check and fill of k (mask and band are filled by the entry).
int blur_args(BlurArgs& k, int h, int w, const Lists& l, int radius, const void* taps, const void* shadow) {
  if (radius < 1 || radius > BLUR_MAX_RADIUS) return fail("blur: a radius of 1..32 pixels");
  if (const int rc = select_args("blur", k.m, h, w, l)) return rc;
  if (!taps || !shadow) return fail("blur: null operand");
  k.taps = static_cast<const int16_t*>(taps), k.radius = radius, k.band = blur_band(radius, 2);
  return 0;
}

// blur_snapshot_k, then blur_k, each on one workgroup per tile of the h x w frame
template <class Dst>
int blur_launch(const BlurArgs& k, const Dst& dst, const Dst& shadow, int pb, void* stream, const char* what) {
  const int grid = ((k.m.h + BTILE - 1) / BTILE) * ((k.m.w + BTILE - 1) / BTILE);
  hipLaunchKernelGGL(blur_snapshot_k<Dst>, dim3(grid), dim3(BT), 0, reinterpret_cast<hipStream_t>(stream), k, dst, shadow);
  if (const int rc = check(what)) return rc;
  hipLaunchKernelGGL(blur_k<Dst>, dim3(grid), dim3(BT), blur_lds(k.band, k.radius, k.radius, pb),
                     reinterpret_cast<hipStream_t>(stream), k, dst, shadow);
  return check(what);
}

// What both chips entries check of the lists, the sizes and the outputs, and fill of k.
int chips_args(ChipArgs& k, int h, int w, const Lists& l, int margin, int capacity, int sh, int sw, void* chips,
               int* rows, int* rects, int* chip_count) {
  if (const int rc = select_args("chips", k.m, h, w, l)) return rc;
  if (!chips || !rows || !rects || !chip_count) return fail("chips: null operand");
  if (sh < 1 || sh > CHIP_MAX_SIDE || sw < 1 || sw > CHIP_MAX_SIDE) return fail("chips: chip sides of 1..256 pixels");
  if (capacity < 1 || capacity > CHIP_MAX_CAPACITY) return fail("chips: a capacity of 1..256 chips");
  if (margin < 0 || margin > CHIP_MAX_MARGIN) return fail("chips: a margin of 0..64 pixels");
  if ((long long)h * w > CHIP_MAX_AREA) return fail("chips: a frame of at most 2^24 pixels (the sums are 32 bits)");
  k.chips = static_cast<uint8_t*>(chips), k.rows = rows, k.rects = rects, k.chip_count = chip_count;
  k.capacity = capacity, k.sh = sh, k.sw = sw, k.margin = margin;
  k.band = std::max(1, std::min(sh, CHIP_NACC * CT / 3 / sw));
  return 0;
}

template <class A>
using ChipKernel = void (*)(ChipArgs, A);

// chips_k on one workgroup per (band of output rows, slot); the LDS is the staged rows and the rows of sums
template <class A>
int chips_launch(ChipKernel<A> kernel, const ChipArgs& k, const A& n, void* stream, const char* what) {
  const dim3 grid((k.sh + k.band - 1) / k.band, k.capacity);
  const size_t lds = size_t(CHIP_ROWS) * (CHIP_ROWW + 3 * k.sw) * sizeof(uint32_t);
  hipLaunchKernelGGL(kernel, grid, dim3(CT), lds, reinterpret_cast<hipStream_t>(stream), k, n);
  return check(what);
}

// The chips kernel of a checked YUV source, from the table the patch kernel is taken from.
template <class A>
int chips_launch_yuv(const NosYuvSrc& s, const ChipArgs& k, const YuvHdrArgs& n, void* stream) {
  const ChipKernel<A> kernel =
      yuv_dispatch<A>(s, [](auto y) -> ChipKernel<A> { return chips_k<Src::YUV, A, decltype(y)>; });
  return chips_launch(kernel, k, A(n), stream, "chips_yuv");
}

// One storage plane of a rescale whose slots share one lattice: P slots a period, `comps` of them components.
ScalePlane scale_plane(const PlaneArg& s, const PlaneArg& d, int ph, int pw, int PH, int PW, int P, int comps) {
  ScalePlane q{};
  q.src = s.p, q.dst = const_cast<uint8_t*>(d.p), q.spitch = s.pitch, q.dpitch = d.pitch;
  q.ph = ph, q.PH = PH, q.P = P, q.pw[0] = pw, q.PW[0] = PW;
  for (int k = 0; k < comps; ++k) q.slots |= uint32_t(1 | k << 2) << (8 * k);
  q.src_slots = pw * P, q.tiles_x = PW, q.unit = comps == 2 ? 1 : 0;
  return q;
}

// The grid and the launch of both rescale entries: k.pl[0 .. np - 1] hold the planes, tiles_x their periods.
int rescale_launch(ScaleArgs& k, int np, void* stream, const char* what) {
  bool wide = false;
  for (int i = 0; i < np; ++i) {
    ScalePlane& q = k.pl[i];
    for (int c = 0; c < 2; ++c) {
      if (q.PW[c] == 0) continue;
      q.area[c] = uint32_t(q.ph) * uint32_t(q.pw[c]), q.inv[c] = 1.0 / double(q.area[c]);
      wide = wide || (uint64_t(q.area[c]) * (uint64_t(k.mask) + 1) > (1ull << 32));
    }
    const int TP = SCALE_T / q.P;
    q.tiles_x = (q.tiles_x + TP - 1) / TP;
  }
  // a band of 8 rows, halved while the grid would hold fewer than 1024 workgroups
  int grid = 0;
  for (k.band = SCALE_BAND;; k.band /= 2) {
    grid = 0;
    for (int i = 0; i < np; ++i) {
      k.pl[i].bands = (k.pl[i].PH + k.band - 1) / k.band, k.pl[i].first = grid;
      grid += k.pl[i].tiles_x * k.pl[i].bands;
    }
    if (grid >= 1024 || k.band == 1) break;
  }
  for (int i = np; i < 3; ++i) k.pl[i].first = grid;
  hipLaunchKernelGGL(wide ? rescale_k<true> : rescale_k<false>, dim3(grid), dim3(SCALE_T), 0,
                     reinterpret_cast<hipStream_t>(stream), k);
  return check(what);
}

// The sides both rescale entries take, of the source and of the target.
int rescale_sides(int h, int w, int H, int W) {
  const bool ok = h >= 1 && w >= 1 && H >= 1 && W >= 1 && std::max(std::max(h, w), std::max(H, W)) <= SCALE_MAX_SIDE;
  return ok ? 0 : fail("rescale: sides of 1..8192 pixels");
}

bool ranges_meet(const PlaneArg& a, const PlaneArg& b) { return a.lo < b.hi && b.lo < a.hi; }

template <class A>
using ConvKernel = void (*)(ConvArgs, A);

// The target of both convert entries, checked and described: packed pixels (dst, its bounds, pitch and order) or, with
// dyuv, a YUV surface and the 12 integers of its colour rule. pl: its planes, for the test against the source's.
int convert_target(ConvArgs& k, PlaneArg* pl, void* dst, const void* dlo, const void* dhi, long long dpitch,
                   const char* dorder, const NosYuvSrc* dyuv, int H, int W, const int* table) {
  auto plane = [](const PlaneArg& s, int P, int cs, int vs, int unit, uint32_t slots) {
    return ConvPlane{const_cast<uint8_t*>(s.p), s.pitch, slots, P, cs, vs, unit};
  };
  if ((dst == nullptr) == (dyuv == nullptr)) return fail("convert: a packed target or a YUV target");
  if (!dyuv) {
    if (!dorder) return fail("convert: null operand");
    PackedDst d{};
    if (const int rc = packed_dst("convert", d, dst, dlo, dhi, dpitch, dorder, H, W)) return rc;
    const uint32_t slots = uint32_t(CV_BYTE) << (8 * d.r) | uint32_t(CV_BYTE | 1 << 3) << 8 |
                           uint32_t(CV_BYTE | 2 << 3) << (8 * (2 - d.r));
    k.pl[0] = plane(d.s, d.C, 0, 0, 1, slots), pl[0] = d.s;
    k.np = 1, k.sb = 1, k.shift = 0, k.maxcode = 255;
    return 0;
  }
  if (dyuv->size != int(sizeof(NosYuvSrc))) return fail("convert: descriptor size mismatch (NosYuvSrc of another build)");
  if (!table) return fail("convert: a YUV target takes the 12 integers of its colour rule");
  YuvDst d{};
  if (const int rc = yuv_dst("convert", d, *dyuv, H, W)) return rc;
  // 2^-14 fixed point: coefficients below 2^18 in size and offsets of the depth keep every sum in int32
  for (int i = 0; i < 12; ++i) {
    if (i < 9 ? std::abs(table[i]) >= (1 << 18) : (table[i] < 0 || table[i] >= (1 << dyuv->depth)))
      return fail("convert: colour rule: coefficients below 2^18 in size, offsets below 2^depth");
    k.tab[i] = table[i];
  }
  k.sb = d.sb, k.shift = d.shift, k.maxcode = (1 << dyuv->depth) - 1;
  const uint32_t y0 = CV_LUMA, y1 = CV_LUMA | 1 << 3, u = CV_U, v = CV_V;
  if (d.layout == YUV_PACKED) {
    // a macropixel: Y0 U Y1 V, U Y0 V Y1 or Y0 V Y1 U
    const uint32_t slots = d.order == 0 ? (y0 | u << 8 | y1 << 16 | v << 24)
                           : d.order == 1 ? (u | y0 << 8 | v << 16 | y1 << 24) : (y0 | v << 8 | y1 << 16 | u << 24);
    k.pl[0] = plane(d.pl[0], 4, 1, 0, 4, slots), k.np = 1;
  } else {
    const int one = d.sb == 1 ? 4 : 1;  // 8-bit samples of a plane go four to a dword
    k.pl[0] = plane(d.pl[0], 1, 0, 0, one, y0);
    if (d.layout == YUV_SEMI) {
      k.pl[1] = plane(d.pl[1], 2, d.hsub, d.vsub, 2, d.order ? (v | u << 8) : (u | v << 8)), k.np = 2;
    } else {
      k.pl[1] = plane(d.pl[1], 1, d.hsub, d.vsub, one, u), k.pl[2] = plane(d.pl[2], 1, d.hsub, d.vsub, one, v), k.np = 3;
    }
  }
  for (int i = 0; i < k.np; ++i) pl[i] = d.pl[i];
  return 0;
}

// What both convert entries check behind their source (sp: its ns planes) and their target, then the grid and the
// launch of the source's two kernels: SAME at equal sizes, else the resampling one on at most 2^24 source pixels.
template <class A>
int convert_launch(ConvKernel<A> same, ConvKernel<A> resample, ConvArgs& k, const A& n, const PlaneArg* sp, int ns,
                   const PlaneArg* dp, int h, int w, int H, int W, void* stream, const char* what) {
  for (int i = 0; i < ns; ++i)
    for (int j = 0; j < k.np; ++j)
      if (ranges_meet(sp[i], dp[j])) return fail(what, ": the source's and the target's storage meet");
  const bool eq = h == H && w == W;
  if (!eq && (long long)h * w > CV_MAX_AREA)
    return fail(what, ": resizing takes a frame of at most 2^24 pixels (the sums are 32 bits)");
  k.h = h, k.w = w, k.H = H, k.W = W, k.tiles_x = (W + CV_TW - 1) / CV_TW;
  // a band of 8 rows, halved while the grid would hold fewer than 1024 workgroups; origins stay even
  int grid = 0;
  for (k.band = CV_BAND;; k.band /= 2) {
    grid = k.tiles_x * ((H + k.band - 1) / k.band);
    if (grid >= 1024 || k.band == 2) break;
  }
  hipLaunchKernelGGL(eq ? same : resample, dim3(grid), dim3(CV_T), 0, reinterpret_cast<hipStream_t>(stream), k, n);
  return check(what);
}

// The two kernels of a checked YUV source, from the table the patch kernel and the chips are taken from.
template <class A>
int convert_launch_yuv(const NosYuvSrc& s, ConvArgs& k, const YuvHdrArgs& n, int ns, const PlaneArg* dp, int h, int w,
                       int H, int W, void* stream) {
  const ConvKernel<A> same =
      yuv_dispatch<A>(s, [](auto y) -> ConvKernel<A> { return convert_k<Src::YUV, A, decltype(y), true>; });
  const ConvKernel<A> resample =
      yuv_dispatch<A>(s, [](auto y) -> ConvKernel<A> { return convert_k<Src::YUV, A, decltype(y), false>; });
  return convert_launch<A>(same, resample, k, A(n), n.pl, ns, dp, h, w, H, W, stream, "convert_yuv");
}

// The sides both convert entries take.
int convert_sides(int h, int w, int H, int W) {
  const bool ok = h >= 1 && w >= 1 && H >= 1 && W >= 1 && std::max(std::max(h, w), std::max(H, W)) <= CV_MAX_SIDE;
  return ok ? 0 : fail("convert: sides of 1..8192 pixels");
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
  OverlayArgs k{};
  const Lists l{count, scores, labels, boxes, track_id, track_hits, modes, N, L, min_hits};
  if (const int rc = overlay_args(k, h, w, l, codes, K, font, thickness, scale)) return rc;
  PackedDst dst{};
  if (const int rc = packed_dst("overlay_packed", dst, img, lo, hi, pitch, order, h, w)) return rc;
  return overlay_launch(k, dst, stream, "overlay_packed");
}

// The same into the one h x w frame of any YUV surface NosYuvSrc describes (tab, chroma and siting are not read): the
// luma sample of every painted pixel, and a chroma sample where its top-left luma pixel is painted; 16-bit samples as
// whole words, code << shift. codes holds Y, U, V codes of the surface's depth. Every check of the descriptor that
// nos_image_patch_planes_yuv makes of its planes, the first and last sample of each inside its [lo, hi).
int nos_overlay_yuv(const NosYuvSrc* dst, int h, int w, const int* count, const float* scores, const int* labels,
                    const float* boxes, const int* track_id, const int* track_hits, int N, const void* modes, int L,
                    const int* codes, int K, const int* font, int thickness, int scale, int min_hits, void* stream) {
  if (const int rc = yuv_open("overlay", "overlay_yuv", dst)) return rc;
  OverlayArgs k{};
  const Lists l{count, scores, labels, boxes, track_id, track_hits, modes, N, L, min_hits};
  if (const int rc = overlay_args(k, h, w, l, codes, K, font, thickness, scale)) return rc;
  YuvDst d{};
  if (const int rc = yuv_dst("overlay_yuv", d, *dst, h, w)) return rc;
  return overlay_launch(k, d, stream, "overlay_yuv");
}

int nos_mosaic_tile_rows() { return MTILE; }
int nos_mosaic_tile_columns() { return MTILE; }

// The detections of the labels select [L] (uint8, non-zero: pixelate) marks, pixelated in packed pixels img: every cell
// of cell x cell pixels (4, 8, 16, 32 or 64, on the lattice from pixel (0, 0)) that a selected row's rectangle touches
// gets, per colour byte, the rounded mean of its bytes inside the frame (image_mosaic.h). The image, the lists and the
// checks are nos_overlay_packed's; nothing is launched unless every check passes, and no byte outside the marked cells'
// colour bytes is written.
int nos_mosaic_packed(void* img, const void* lo, const void* hi, long long pitch, const char* order, int h, int w,
                      const int* count, const float* scores, const int* labels, const float* boxes,
                      const int* track_id, const int* track_hits, int N, const void* select, int L, int min_hits,
                      int cell, void* stream) {
  if (!img || !order) return fail("mosaic: null operand");
  MosaicArgs k{};
  const Lists l{count, scores, labels, boxes, track_id, track_hits, select, N, L, min_hits};
  if (const int rc = mosaic_args(k, h, w, l, cell)) return rc;
  PackedDst dst{};
  if (const int rc = packed_dst("mosaic_packed", dst, img, lo, hi, pitch, order, h, w)) return rc;
  return mosaic_launch(k, dst, stream, "mosaic_packed");
}

// The same in the one h x w frame of any YUV surface NosYuvSrc describes, as nos_overlay_yuv takes it: per sample plane
// the mean of the codes ((word >> shift) & (2^depth - 1) of a 16-bit sample) whose owner pixel lies in the cell, stored
// to every one of them, 16-bit samples as whole words.
int nos_mosaic_yuv(const NosYuvSrc* dst, int h, int w, const int* count, const float* scores, const int* labels,
                   const float* boxes, const int* track_id, const int* track_hits, int N, const void* select, int L,
                   int min_hits, int cell, void* stream) {
  if (const int rc = yuv_open("mosaic", "mosaic_yuv", dst)) return rc;
  MosaicArgs k{};
  const Lists l{count, scores, labels, boxes, track_id, track_hits, select, N, L, min_hits};
  if (const int rc = mosaic_args(k, h, w, l, cell)) return rc;
  YuvDst d{};
  if (const int rc = yuv_dst("mosaic_yuv", d, *dst, h, w)) return rc;
  k.mask = (1 << dst->depth) - 1;
  return mosaic_launch(k, d, stream, "mosaic_yuv");
}

int nos_blur_max_radius() { return BLUR_MAX_RADIUS; }

// The bytes of the shadow nos_blur_packed takes for an image of h x w pixels of the order's bytes at `pitch`; -1 for an
// unknown order or a pitch below a row's bytes.
long long nos_blur_shadow_packed(long long pitch, const char* order, int h, int w) {
  PackedArgs o{};
  const int C = order ? packed_order(order, o) : 0;
  if (!C || h <= 0 || w <= 0 || pitch < (long long)w * C) return fail("blur_packed: the shadow of an unknown image");
  const PlaneArg pl = plane_arg(nullptr, nullptr, nullptr, pitch, 0);
  return blur_shadow(&pl, PlaneSizes{1, {h}, {(long long)w * C}}, nullptr, nullptr);
}

// The same for the surface nos_blur_yuv takes.
long long nos_blur_shadow_yuv(const NosYuvSrc* dst, int h, int w) {
  if (!dst || dst->size != int(sizeof(NosYuvSrc))) return fail("blur_yuv: descriptor size mismatch (NosYuvSrc of another build)");
  YuvDst d{};
  if (const int rc = yuv_dst("blur_yuv", d, *dst, h, w)) return rc;
  return blur_shadow(d.pl, yuv_sizes(*dst, h, w), nullptr, nullptr);
}

// The detections of the labels select [L] (uint8, non-zero: blur) marks, blurred in packed pixels img: every pixel of a
// selected row's rectangle gets, per colour byte, the separable Gaussian of integer taps (taps: int16 [2][65] on the
// device, the taps of `radius` and of radius >> 1, each summing to 256) over the bytes the image held before the call,
// indices clamped at its edges (image_blur.h). shadow: shadow_bytes >= nos_blur_shadow_packed's of device memory the
// call may overwrite. The image, the lists and the checks are nos_mosaic_packed's; nothing is launched unless every
// check passes, and no byte outside the painted pixels' colour bytes is written.
int nos_blur_packed(void* img, const void* lo, const void* hi, long long pitch, const char* order, int h, int w,
                    const int* count, const float* scores, const int* labels, const float* boxes, const int* track_id,
                    const int* track_hits, int N, const void* select, int L, int min_hits, int radius, const void* taps,
                    void* shadow, long long shadow_bytes, void* stream) {
  if (!img || !order) return fail("blur: null operand");
  BlurArgs k{};
  const Lists l{count, scores, labels, boxes, track_id, track_hits, select, N, L, min_hits};
  if (const int rc = blur_args(k, h, w, l, radius, taps, shadow)) return rc;
  PackedDst dst{};
  if (const int rc = packed_dst("blur_packed", dst, img, lo, hi, pitch, order, h, w)) return rc;
  PackedDst sh = dst;
  if (blur_shadow(&dst.s, PlaneSizes{1, {h}, {(long long)w * dst.C}}, shadow, &sh.s) > shadow_bytes)
    return fail("blur_packed: the shadow is smaller than nos_blur_shadow_packed asks");
  return blur_launch(k, dst, sh, 2, stream, "blur_packed");
}

// The same in the one h x w frame of any YUV surface NosYuvSrc describes, as nos_mosaic_yuv takes it: per sample plane
// the codes ((word >> shift) & (2^depth - 1) of a 16-bit sample) blurred at the plane's own resolution with the taps of
// radius >> hsub and radius >> vsub, stored where the sample's owner pixel is painted, 16-bit samples as whole words.
int nos_blur_yuv(const NosYuvSrc* dst, int h, int w, const int* count, const float* scores, const int* labels,
                 const float* boxes, const int* track_id, const int* track_hits, int N, const void* select, int L,
                 int min_hits, int radius, const void* taps, void* shadow, long long shadow_bytes, void* stream) {
  if (const int rc = yuv_open("blur", "blur_yuv", dst)) return rc;
  BlurArgs k{};
  const Lists l{count, scores, labels, boxes, track_id, track_hits, select, N, L, min_hits};
  if (const int rc = blur_args(k, h, w, l, radius, taps, shadow)) return rc;
  YuvDst d{};
  if (const int rc = yuv_dst("blur_yuv", d, *dst, h, w)) return rc;
  YuvDst sh = d;
  if (blur_shadow(d.pl, yuv_sizes(*dst, h, w), shadow, sh.pl) > shadow_bytes)
    return fail("blur_yuv: the shadow is smaller than nos_blur_shadow_yuv asks");
  const int pb = dst->sample_bytes == 2 ? 4 : 2;
  k.m.mask = (1 << dst->depth) - 1, k.band = blur_band(radius, pb);
  return blur_launch(k, d, sh, pb, stream, "blur_yuv");
}

int nos_chips_max_side() { return CHIP_MAX_SIDE; }
int nos_chips_max_capacity() { return CHIP_MAX_CAPACITY; }
int nos_chips_max_margin() { return CHIP_MAX_MARGIN; }
int nos_chips_column_chunk() { return 4 * CHIP_GROUPS; }
int nos_chips_row_chunk() { return CHIP_ROWS; }

// The detections of the labels select [L] (uint8, non-zero: cut) marks, cut out of packed pixels img [h][w][C] (order,
// pitch and [lo, hi) as in nos_image_patch_planes_packed; a crop view is read in place): the rows the rule selects
// (nos_mosaic_packed's lists and filters; the rectangle grown by `margin` pixels and clipped to the frame, dropped when
// nothing is left) take slots 0, 1, ... in row order, and each of the first `capacity` gets chips [slot] [sh][sw][3]
// uint8, the exact area average of its rectangle stretched to sh x sw (image_chips.h), rows [slot] its row and rects
// [slot] its rectangle (X0, Y0, X1, Y1), exclusive; the other slots get -1, zeros and a chip of zeros; chip_count [1]
// the slots used. All outputs are device memory, int32 but the chips. Nothing is launched unless every check passes.
int nos_chips_packed(const void* img, const void* lo, const void* hi, long long pitch, const char* order, int h, int w,
                     const int* count, const float* scores, const int* labels, const float* boxes, const int* track_id,
                     const int* track_hits, int N, const void* select, int L, int min_hits, int margin, int capacity,
                     int sh, int sw, void* chips, int* rows, int* rects, int* chip_count, void* stream) {
  if (!img || !order) return fail("chips: null operand");
  ChipArgs k{};
  const Lists l{count, scores, labels, boxes, track_id, track_hits, select, N, L, min_hits};
  if (const int rc = chips_args(k, h, w, l, margin, capacity, sh, sw, chips, rows, rects, chip_count)) return rc;
  PackedDst d{};
  if (const int rc = packed_dst("chips_packed", d, const_cast<void*>(img), lo, hi, pitch, order, h, w)) return rc;
  const PackedArgs n{d.s, d.r, 1, 2 - d.r};
  if (d.C == 4) return chips_launch(chips_k<Src::PACKED4, PackedArgs>, k, n, stream, "chips_packed");
  return chips_launch(chips_k<Src::PACKED3, PackedArgs>, k, n, stream, "chips_packed");
}

// The same out of the one h x w frame of any YUV source NosYuvSrc describes, converted as nos_image_patch_planes_yuv
// converts it (nearest or bilinear chroma at its siting) or, with hdr not null, as nos_image_patch_planes_yuv_hdr does
// (PQ / HLG through the tables). Every check those entries make of the descriptor, the planes and the tables.
int nos_chips_yuv(const NosYuvSrc* src, const NosYuvHdr* hdr, int h, int w, const int* count, const float* scores,
                  const int* labels, const float* boxes, const int* track_id, const int* track_hits, int N,
                  const void* select, int L, int min_hits, int margin, int capacity, int sh, int sw, void* chips,
                  int* rows, int* rects, int* chip_count, void* stream) {
  if (const int rc = yuv_open("chips", "chips_yuv", src)) return rc;
  if (hdr && hdr->size != int(sizeof(NosYuvHdr)))
    return fail("chips_yuv: table descriptor size mismatch (NosYuvHdr of another build)");
  ChipArgs k{};
  const Lists l{count, scores, labels, boxes, track_id, track_hits, select, N, L, min_hits};
  if (const int rc = chips_args(k, h, w, l, margin, capacity, sh, sw, chips, rows, rects, chip_count)) return rc;
  YuvHdrArgs n{};
  if (yuv_source(*src, n, 1, h, w) || (hdr && hdr_args(*src, *hdr, n))) return fail("chips_yuv", ": the source: " + g_err);
  if (hdr) return chips_launch_yuv<YuvHdrArgs>(*src, k, n, stream);
  if (src->chroma == 1) return chips_launch_yuv<YuvBilinearArgs>(*src, k, n, stream);
  return chips_launch_yuv<YuvArgs>(*src, k, n, stream);
}

int nos_rescale_row_chunk() { return SCALE_ROWS; }
int nos_rescale_column_chunk() { return SCALE_SLOTS; }
int nos_rescale_tile() { return SCALE_T; }
int nos_rescale_max_side() { return SCALE_MAX_SIDE; }

// The packed pixels src [h][w][C] resized into dst [H][W][C] of the same order (pitches and [lo, hi) as in
// nos_overlay_packed; crop views are read and written in place): every colour byte of dst is the exact area average
// of its component (image_scale.h), the fourth byte of a four-byte pixel is neither read into a result nor written.
// Sides of 1..8192; the two storage ranges must not meet. Nothing is launched unless every check passes.
int nos_rescale_packed(const void* src, const void* slo, const void* shi, long long spitch, int h, int w, void* dst,
                       const void* dlo, const void* dhi, long long dpitch, int H, int W, const char* order,
                       void* stream) {
  if (!src || !dst || !order) return fail("rescale: null operand");
  if (const int rc = rescale_sides(h, w, H, W)) return rc;
  PackedDst s{}, d{};
  if (const int rc = packed_dst("rescale_packed", s, const_cast<void*>(src), slo, shi, spitch, order, h, w)) return rc;
  if (const int rc = packed_dst("rescale_packed", d, dst, dlo, dhi, dpitch, order, H, W)) return rc;
  if (ranges_meet(s.s, d.s)) return fail("rescale_packed: the source's and the target's storage meet");
  ScaleArgs k{};
  k.pl[0] = scale_plane(s.s, d.s, h, w, H, W, s.C, 3);
  k.sb = 1, k.shift = 0, k.mask = 255;
  return rescale_launch(k, 1, stream, "rescale_packed");
}

// The same between the one h x w frame src and the one H x W frame dst of a YUV surface (the checks of
// nos_overlay_yuv on either side): both descriptors agree in layout, subsampling, sample format and order; every
// sample plane is resized on its own lattice, a 16-bit sample stored whole as code << shift.
int nos_rescale_yuv(const NosYuvSrc* src, int h, int w, const NosYuvSrc* dst, int H, int W, void* stream) {
  if (!src || !dst) return fail("rescale: null operand");
  if (src->size != int(sizeof(NosYuvSrc)) || dst->size != int(sizeof(NosYuvSrc)))
    return fail("rescale_yuv: descriptor size mismatch (NosYuvSrc of another build)");
  if (const int rc = rescale_sides(h, w, H, W)) return rc;
  YuvDst s{}, d{};
  if (const int rc = yuv_dst("rescale_yuv", s, *src, h, w)) return rc;
  if (const int rc = yuv_dst("rescale_yuv", d, *dst, H, W)) return rc;
  if (s.layout != d.layout || s.hsub != d.hsub || s.vsub != d.vsub || s.sb != d.sb || src->depth != dst->depth ||
      s.shift != d.shift || s.order != d.order)
    return fail("rescale_yuv: the source and the target differ in layout, subsampling, sample format or order");
  const PlaneSizes zs = yuv_sizes(*src, h, w), zd = yuv_sizes(*dst, H, W);
  const int np = zs.np, ch = int(zs.ch), cw = int(zs.cw), CH = int(zd.ch), CW = int(zd.cw);
  for (int i = 0; i < np; ++i)
    for (int j = 0; j < np; ++j)
      if (ranges_meet(s.pl[i], d.pl[j])) return fail("rescale_yuv: the source's and the target's storage meet");
  ScaleArgs k{};
  k.sb = s.sb, k.shift = s.shift, k.mask = (1 << src->depth) - 1;
  if (s.layout == YUV_PACKED) {
    // a macropixel: luma (class 0, two columns) at slots yo and yo + 2, the chroma components (class 1) at the others
    ScalePlane& q = k.pl[0];
    q = scale_plane(s.pl[0], d.pl[0], h, w, H, W, 4, 0);
    q.pw[1] = cw, q.PW[1] = CW, q.ns[0] = 1, q.src_slots = 4 * cw, q.tiles_x = CW, q.unit = 2;
    const int yo = s.order == 1 ? 1 : 0;
    for (int slot = 0; slot < 4; ++slot) {
      const bool luma = (slot & 1) == yo;
      q.slots |= uint32_t(luma ? (1 | yo << 2 | (slot >> 1) << 4) : (2 | slot << 2)) << (8 * slot);
    }
  } else {
    k.pl[0] = scale_plane(s.pl[0], d.pl[0], h, w, H, W, 1, 1);
    if (s.layout == YUV_SEMI) {
      k.pl[1] = scale_plane(s.pl[1], d.pl[1], ch, cw, CH, CW, 2, 2);
    } else {
      for (int i = 1; i < 3; ++i) k.pl[i] = scale_plane(s.pl[i], d.pl[i], ch, cw, CH, CW, 1, 1);
    }
  }
  return rescale_launch(k, np, stream, "rescale_yuv");
}

int nos_convert_max_side() { return CV_MAX_SIDE; }
int nos_convert_tile() { return CV_TW; }
int nos_convert_row_chunk() { return CV_ROWS; }
int nos_convert_column_chunk() { return 4 * CV_GROUPS; }

// The packed pixels img [h][w][C] (as nos_chips_packed takes them) converted into a second surface of any SDR layout
// at H x W (convert_k, image_convert.h): R, the exact area average of the frame stretched to H x W (the frame itself at
// equal sizes), stored as packed pixels dst [H][W][C'] in dorder (as nos_rescale_packed takes its target; the fourth
// byte is not written) or, with dyuv, as the YUV surface it describes (as nos_rescale_yuv takes its target) by the 12
// integers of table (ops/image.py's convert_table: luma per pixel, chroma from the mean of its block). Exactly one of
// dst and dyuv is given. Sides of 1..8192, a source of at most 2^24 pixels unless the sizes are equal; the two storage
// ranges must not meet. Every sample of the target is written, nothing else. Nothing is launched unless every check
// passes.
int nos_convert_packed(const void* img, const void* lo, const void* hi, long long pitch, const char* order, int h, int w,
                       void* dst, const void* dlo, const void* dhi, long long dpitch, const char* dorder,
                       const NosYuvSrc* dyuv, int H, int W, const int* table, void* stream) {
  if (!img || !order) return fail("convert: null operand");
  if (const int rc = convert_sides(h, w, H, W)) return rc;
  PackedDst s{};
  if (const int rc = packed_dst("convert_packed", s, const_cast<void*>(img), lo, hi, pitch, order, h, w)) return rc;
  ConvArgs k{};
  PlaneArg dp[3];
  if (const int rc = convert_target(k, dp, dst, dlo, dhi, dpitch, dorder, dyuv, H, W, table)) return rc;
  const PackedArgs n{s.s, s.r, 1, 2 - s.r};
  if (s.C == 4)
    return convert_launch<PackedArgs>(convert_k<Src::PACKED4, PackedArgs, NoYuv, true>,
                                      convert_k<Src::PACKED4, PackedArgs, NoYuv, false>, k, n, &s.s, 1, dp, h, w, H, W,
                                      stream, "convert_packed");
  return convert_launch<PackedArgs>(convert_k<Src::PACKED3, PackedArgs, NoYuv, true>,
                                    convert_k<Src::PACKED3, PackedArgs, NoYuv, false>, k, n, &s.s, 1, dp, h, w, H, W,
                                    stream, "convert_packed");
}

// The same from the one h x w frame of any YUV source NosYuvSrc describes, read as nos_chips_yuv reads it (nearest or
// bilinear chroma at its siting; with hdr not null, PQ / HLG through the tables).
int nos_convert_yuv(const NosYuvSrc* src, const NosYuvHdr* hdr, int h, int w, void* dst, const void* dlo, const void* dhi,
                    long long dpitch, const char* dorder, const NosYuvSrc* dyuv, int H, int W, const int* table,
                    void* stream) {
  if (const int rc = yuv_open("convert", "convert_yuv", src)) return rc;
  if (hdr && hdr->size != int(sizeof(NosYuvHdr)))
    return fail("convert_yuv: table descriptor size mismatch (NosYuvHdr of another build)");
  if (const int rc = convert_sides(h, w, H, W)) return rc;
  YuvHdrArgs n{};
  if (yuv_source(*src, n, 1, h, w) || (hdr && hdr_args(*src, *hdr, n))) return fail("convert_yuv", ": the source: " + g_err);
  ConvArgs k{};
  PlaneArg dp[3];
  if (const int rc = convert_target(k, dp, dst, dlo, dhi, dpitch, dorder, dyuv, H, W, table)) return rc;
  const int ns = yuv_sizes(*src, h, w).np;
  if (hdr) return convert_launch_yuv<YuvHdrArgs>(*src, k, n, ns, dp, h, w, H, W, stream);
  if (src->chroma == 1) return convert_launch_yuv<YuvBilinearArgs>(*src, k, n, ns, dp, h, w, H, W, stream);
  return convert_launch_yuv<YuvArgs>(*src, k, n, ns, dp, h, w, H, W, stream);
}

int nos_features_max_stripes() { return FEAT_MAX_STRIPES; }
int nos_features_max_shift() { return FEAT_MAX_SHIFT; }

// One colour descriptor per chip (chip_features_k, image_features.h): chips [capacity][sh][sw][3] uint8 and rows
// [capacity] int32 as the chips entries write them -> features [capacity][64 stripes] int32, zeros for a slot whose row is
// negative; every element is written. stripes: 1, 2, 4 or 8, at most sh.
int nos_chip_features(const void* chips, const int* rows, int capacity, int sh, int sw, int stripes, int* features,
                      void* stream) {
  if (!chips || !rows || !features) return fail("chip_features: null operand");
  if (sh < 1 || sh > CHIP_MAX_SIDE || sw < 1 || sw > CHIP_MAX_SIDE) return fail("chip_features: chip sides of 1..256 pixels");
  if (capacity < 1 || capacity > CHIP_MAX_CAPACITY) return fail("chip_features: a capacity of 1..256 chips");
  if ((stripes != 1 && stripes != 2 && stripes != 4 && stripes != 8) || stripes > sh)
    return fail("chip_features: 1, 2, 4 or 8 stripes, no more than the chip has rows");
  hipLaunchKernelGGL(chip_features_k, dim3(stripes, capacity), dim3(FT), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(chips), rows, sh, sw, stripes, features);
  return check("chip_features");
}

// Histogram intersection (feature_overlap_k): F [K][D], G [T][D] int32 -> S [K][T] int32, S[k][t] = sum_d min(F, G);
// every element is written. D is a multiple of 64 up to 512, both matrices start on a 16-byte boundary.
int nos_feature_overlap(const int* F, const int* G, int K, int T, int D, int* S, void* stream) {
  if (!F || !G || !S) return fail("feature_overlap: null operand");
  if (K < 1 || K > OV_MAX_K || T < 1 || T > OV_MAX_T) return fail("feature_overlap: 1..256 chips against 1..1024 tracks");
  if (D < OV_D || D > FEAT_MAX_D || D % OV_D) return fail("feature_overlap: a length of 64, 128, ... 512");
  if ((reinterpret_cast<uintptr_t>(F) | reinterpret_cast<uintptr_t>(G)) & 15)
    return fail("feature_overlap: the matrices start on a 16-byte boundary");
  hipLaunchKernelGGL(feature_overlap_k, dim3((T + OV_TT - 1) / OV_TT, (K + OV_TK - 1) / OV_TK), dim3(FT), 0,
                     reinterpret_cast<hipStream_t>(stream), F, G, K, T, D, S);
  return check("feature_overlap");
}

// nos_track_update_f32 with appearance (track_update_app_f32): besides its operands S [K][T] int32 as
// nos_feature_overlap writes it from this frame's descriptors and the state's, rows [K] the chips' rows, has [T] and
// src [T] of the state; gate_q and reid_q the thresholds on S (reid 0: no re-identification).
int nos_track_update_app_f32(const int* count, const float* scores, const int* labels, const float* boxes, int N,
                             float* t_boxes, float* t_vel, int* t_labels, int* t_ids, int* t_hits, int* t_misses,
                             int* next_id, int* dropped, int T, float match_threshold, int max_age, float birth_threshold,
                             int motion, float velocity_gain, int* track_id, int* track_hits, const int* S,
                             const int* rows, int K, int* has, int* src, int gate_q, int reid_q, int reid, void* stream) {
  if (!count || !scores || !labels || !boxes || !t_boxes || !t_vel || !t_labels || !t_ids || !t_hits || !t_misses ||
      !next_id || !dropped || !track_id || !track_hits || !S || !rows || !has || !src)
    return fail("track_update: null operand");
  if (N <= 0 || N > MMAX || T <= 0 || T > TMAX) return fail("track_update: 0 < rows <= 1024, 0 < slots <= 1024");
  if (K < 1 || K > OV_MAX_K) return fail("track_update: 1..256 chip slots");
  if (motion != 0 && motion != 1) return fail("track_update: the motion is 0 (none) or 1 (constant)");
  if (!(match_threshold >= 0.f) || max_age < 0 || !(velocity_gain >= 0.f && velocity_gain <= 1.f))
    return fail("track_update: match_threshold >= 0, max_age >= 0, 0 <= velocity_gain <= 1");
  if (gate_q < 0 || reid_q < 0 || (reid != 0 && reid != 1)) return fail("track_update: thresholds on S from 0 up");
  const TrackApp ap{S, rows, has, src, K, gate_q, reid_q, reid};
  hipLaunchKernelGGL(track_update_app_f32, dim3(1), dim3(DT), 0, reinterpret_cast<hipStream_t>(stream), count, scores,
                     labels, boxes, N, t_boxes, t_vel, t_labels, t_ids, t_hits, t_misses, next_id, dropped, T,
                     match_threshold, max_age, birth_threshold, motion, velocity_gain, track_id, track_hits, ap);
  return check("track_update_app_f32");
}

// The descriptors the tracks keep (track_features_k), after nos_track_update_app_f32: features [K][D] of this frame's
// chips, ids / src [T] of the state -> feat [T][D] and has [T] updated in place with 2^-shift of the new descriptor.
int nos_track_features(const int* features, int K, int D, const int* ids, const int* src, int T, int* feat, int* has,
                       int shift, void* stream) {
  if (!features || !ids || !src || !feat || !has) return fail("track_features: null operand");
  if (K < 1 || K > OV_MAX_K || T < 1 || T > TMAX || D < 1 || D > FEAT_MAX_D)
    return fail("track_features: 1..256 chips, 1..1024 slots, a length up to 512");
  if (shift < 0 || shift > FEAT_MAX_SHIFT) return fail("track_features: a shift of 0..8");
  hipLaunchKernelGGL(track_features_k, dim3(T), dim3(128), 0, reinterpret_cast<hipStream_t>(stream), features, K, D, ids,
                     src, feat, has, shift);
  return check("track_features");
}

}  // extern "C"
