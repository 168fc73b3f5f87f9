// The detections behind the model, for the image library (image.hip): the wave reductions, the per-row score pass,
// box_overlap and the two kernels.
//  * detections_f32 — softmax over the class logits, the best of the first L classes, the box in
//    corner format scaled to the original image, and a stable compaction of the rows above the
//    threshold; one workgroup per image, one wave per row.
//  * merge_detections_f32 — the detections of B overlapping tiles of one frame as one list: scores as above, boxes in
//    frame pixels, the candidates ordered by score (a rank count in LDS), duplicates of another tile's kept box
//    suppressed greedily (one pivot per barrier), the kept rows compacted in that order; one workgroup.
// Included by image.hip alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace {
constexpr int MMAX = 1024, CMAX = 128;
// the detections workgroup: 16 waves, so the 100 rows of YOLOS are 7 dependent row passes, not 25
constexpr int DT = 1024, DW = DT / 64;

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

// One wave's pass over a row x of C logits (C <= 128: two per lane): the softmax, and the largest probability of the
// first L = C - 1 classes and its index, written to *score and *label
__device__ __forceinline__ void row_best(const float* x, int C, int L, int lane, float* score, int* label) {
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
    *score = best;
    *label = idx;
  }
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
    row_best(logits + (size_t(b) * M + row) * C, C, L, lane, s_score + row, s_label + row);
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
    row_best(logits + size_t(row) * C, C, L, lane, s_score + row, s_label + row);
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
}  // namespace
