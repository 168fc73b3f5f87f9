// The write side of the image library (image.hip): one frame's detections painted into the frame's own planes.
//  * overlay_k<Surface> — a frame-tile rasteriser, one workgroup per OTH x OTW tile of luma pixels, so the grid
//    depends on the frame's size alone and nothing on `count` at launch. A workgroup turns the n rows into integer
//    records (make_record: the drawing rule's filters, the outer rectangle, the tag's digits, the colour slot), keeps
//    those that touch its tile in an LDS list in row order (a ballot compaction per 256 rows) and, where the list is
//    not empty, finds for each of its pixels the first listed row that covers it (cover) and stores that pixel's
//    samples (PackedDst / YuvDst: store).
// The rule is exact integers; ops/image.py's overlay_reference states it in full. Every sample belongs to one luma
// pixel — a chroma sample to the luma pixel at its top-left — and is stored only by that pixel's thread, behind the
// guard y < h && x < w; nothing is read back, no address is clamped, every store is a plain store of a whole sample.
// Included by image.hip alone, after image_stage.h (PlaneArg).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "image_stage.h"

namespace {
// threads of a workgroup; the tile of luma pixels it paints (a thread: 2 columns of OTH / 8 rows); rows of a list
constexpr int OT = 256, OTH = 32, OTW = 64, OMAX = 1024;
// the largest thickness, tag scale and colour count the host lets through: no sum of a clamped coordinate (2^20 in
// size), a thickness and a tag's extent (55 * scale) leaves int32
constexpr int OVERLAY_MAX_T = 1 << 20, OVERLAY_MAX_S = 1 << 10, OVERLAY_MAX_K = 1 << 10;
constexpr float OVERLAY_CLAMP = 1048576.f;
static_assert(OT == 8 * (OTW / 2) && OTH % 8 == 0, "a pass of the raster loop is 8 rows of pixel pairs");

// One frame's lists as detections_f32 / merge_detections_f32 write them, ids and hits as track_update_f32 does (both
// null: no ids), and the tables, all on the device: modes [L] (0 not drawn, 1 outline and tag, 2 redacted), codes
// [2 K + 1][3] (fill and text colour of palette entry k at 2 k and 2 k + 1, the redact colour last; a colour is the
// surface's three codes: R, G, B bytes or Y, U, V), font [10][7] (a digit's rows, bit 4 the leftmost column).
struct OverlayArgs {
  const int* count;
  const float* scores;
  const int* labels;
  const float* boxes;
  const int* track_id;
  const int* track_hits;
  const uint8_t* modes;
  const int* codes;
  const int* font;
  int N, L, K, t, s, min_hits, h, w;
};

// A drawn row. (x0, y0)..(x1, y1): the outer rectangle, inclusive; ty: the tag's first row; tag: digit j (most
// significant first) in bits 4 j .. 4 j + 3, their number in bits 24..26 (0: no tag), the mode in bits 28..29;
// col: the colour slot of the fill (the text's is the next one).
struct OverlayRec {
  int x0, y0, x1, y1, ty, tag, col;
};

// Row r as a record; false when the rule does not draw it.
__device__ __forceinline__ bool make_record(const OverlayArgs& a, int r, OverlayRec& q) {
  if (!(a.scores[r] > 0.f)) return false;  // a NaN is not drawn
  const int label = a.labels[r];
  if (label < 0 || label >= a.L) return false;
  const int mode = a.modes[label];
  if (mode != 1 && mode != 2) return false;
  int key = label;
  if (a.track_id != nullptr) {
    key = a.track_id[r];
    if (key <= 0 || a.track_hits[r] < a.min_hits) return false;
  }
  float c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c[i] = a.boxes[4 * size_t(r) + i];
    if (!isfinite(c[i])) return false;
    c[i] = fminf(fmaxf(c[i], -OVERLAY_CLAMP), OVERLAY_CLAMP);
  }
  q.x0 = int(floorf(c[0])), q.y0 = int(floorf(c[1]));
  q.x1 = int(ceilf(c[2])) - 1, q.y1 = int(ceilf(c[3])) - 1;
  if (q.x1 < q.x0 || q.y1 < q.y0) return false;
  q.ty = q.y0, q.tag = mode << 28, q.col = 2 * a.K;
  if (mode == 1) {
    q.col = 2 * (key % a.K);
    if (a.s > 0) {
      const int v = key % 1000000;
      int nd = 1;
      for (int p = 10; p <= v; p *= 10) ++nd;  // v < 10^6: p stops at 10^6
      int rest = v;
      for (int j = nd - 1; j >= 0; --j) {
        q.tag |= (rest % 10) << (4 * j);
        rest /= 10;
      }
      q.tag |= nd << 24;
      if (q.y0 - 9 * a.s >= 0) q.ty = q.y0 - 9 * a.s;
    }
  }
  return true;
}

// The colour slot record q gives pixel (x, y), or -1 when it does not cover it; font: the table in LDS.
__device__ __forceinline__ int cover(const OverlayRec& q, int x, int y, int t, int s, const int* font) {
  const bool outer = x >= q.x0 && x <= q.x1 && y >= q.y0 && y <= q.y1;
  if ((q.tag >> 28) == 2) return outer ? q.col : -1;
  const int nd = (q.tag >> 24) & 7;
  if (nd != 0) {
    const int u = x - q.x0, v = y - q.ty;
    if (u >= 0 && u < (6 * nd + 1) * s && v >= 0 && v < 9 * s) {
      const int gu = u - s, gv = v - s;
      if (gu >= 0 && gu < 6 * s * nd && gv >= 0 && gv < 7 * s) {
        const int cu = (gu % (6 * s)) / s;
        if (cu < 5 && ((font[((q.tag >> (4 * (gu / (6 * s)))) & 15) * 7 + gv / s] >> (4 - cu)) & 1)) return q.col + 1;
      }
      return q.col;
    }
  }
  const bool inner = x >= q.x0 + t && x <= q.x1 - t && y >= q.y0 + t && y <= q.y1 - t;
  return outer && !inner ? q.col : -1;
}

// Packed pixels of C bytes, red at byte r and blue at byte 2 - r; a fourth byte is never written.
struct PackedDst {
  PlaneArg s;
  int C, r;
  __device__ __forceinline__ void store(int y, int x, const int* col) const {
    uint8_t* p = const_cast<uint8_t*>(s.p) + y * s.pitch + (long long)x * C;
    p[r] = uint8_t(col[0]), p[1] = uint8_t(col[1]), p[2 - r] = uint8_t(col[2]);
  }
};

// A YUV surface as NosYuvSrc describes it (image_yuv.h: layout 0 planar, 1 semi-planar, 2 packed 4:2:2). A sample is
// one byte, or a 16-bit word written whole as code << shift.
struct YuvDst {
  PlaneArg pl[3];
  int layout, hsub, vsub, sb, shift, order;
  __device__ __forceinline__ void put(int plane, long long row, long long sample, int code) const {
    uint8_t* p = const_cast<uint8_t*>(pl[plane].p) + row * pl[plane].pitch + sample * sb;
    if (sb == 2) *reinterpret_cast<uint16_t*>(p) = uint16_t(code << shift);
    else *p = uint8_t(code);
  }
  __device__ __forceinline__ void store(int y, int x, const int* col) const {
    // the chroma sample whose top-left luma pixel this is
    const bool chroma = (x & ((1 << hsub) - 1)) == 0 && (y & ((1 << vsub) - 1)) == 0;
    const int cy = y >> vsub, cx = x >> hsub;
    if (layout == 2) {
      // a macropixel of four bytes: yuyv (Y0 U Y1 V), uyvy (U Y0 V Y1), yvyu (Y0 V Y1 U)
      const int yo = order == 1 ? 1 : 0, uo = order == 0 ? 1 : order == 1 ? 0 : 3, vo = order == 0 ? 3 : order == 1 ? 2 : 1;
      put(0, y, 4LL * cx + yo + 2 * (x & 1), col[0]);
      if (chroma) put(0, y, 4LL * cx + uo, col[1]), put(0, y, 4LL * cx + vo, col[2]);
    } else {
      put(0, y, x, col[0]);
      if (!chroma) return;
      if (layout == 1) put(1, cy, 2LL * cx + order, col[1]), put(1, cy, 2LL * cx + 1 - order, col[2]);
      else put(1, cy, cx, col[1]), put(2, cy, cx, col[2]);
    }
  }
};

// The trip count of the loop that holds barriers (n, the rows) is read from LDS by all threads, and so is what the
// loop adds to the list's length.
template <class Dst>
__global__ __launch_bounds__(OT) void overlay_k(OverlayArgs a, Dst dst) {
  __shared__ OverlayRec list[OMAX];
  __shared__ int s_font[70], s_wave[OT / 64], s_n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (a.w + OTW - 1) / OTW;
  const int ty0 = int(blockIdx.x) / tiles_x * OTH, tx0 = int(blockIdx.x) % tiles_x * OTW;
  if (tid == 0) s_n = min(max(a.count[0], 0), a.N);
  if (tid < 70) s_font[tid] = a.font[tid];
  __syncthreads();
  const int n = s_n;
  int m = 0;  // rows listed so far: the same in every thread
  for (int base = 0; base < n; base += OT) {
    const int r = base + tid;
    OverlayRec q;
    bool keep = r < n && make_record(a, r, q);
    if (keep) {
      // what the row may paint: the outer rectangle and, with a tag, the tag's
      int right = q.x1, bottom = q.y1;
      const int nd = (q.tag >> 24) & 7;
      if (nd != 0) right = max(right, q.x0 + (6 * nd + 1) * a.s - 1), bottom = max(bottom, q.ty + 9 * a.s - 1);
      keep = q.x0 < tx0 + OTW && right >= tx0 && q.ty < ty0 + OTH && bottom >= ty0;
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    int off = m;
    for (int k = 0; k < OT / 64; ++k) {
      if (k < wave) off += s_wave[k];
      m += s_wave[k];
    }
    if (keep) list[off + __popcll(mask & ((1ull << lane) - 1ull))] = q;
    __syncthreads();  // the list is written, and s_wave is free for the next 256 rows
  }
  if (m == 0) return;
  for (int pass = 0; pass < OTH / 8; ++pass) {
    const int y = ty0 + pass * 8 + tid / (OTW / 2);
    if (y >= a.h) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int x = tx0 + 2 * (tid % (OTW / 2)) + i;
      if (x >= a.w) continue;
      int slot = -1;
      for (int k = 0; k < m && slot < 0; ++k) slot = cover(list[k], x, y, a.t, a.s, s_font);
      if (slot >= 0) dst.store(y, x, a.codes + 3 * slot);
    }
  }
}
}  // namespace
