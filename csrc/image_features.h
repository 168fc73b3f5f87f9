// Appearance for the tracker of the image library (image.hip): what a chip looks like as a fixed-length vector of
// integers, how much two such vectors share, and the vector a track keeps. Three kernels, all exact in int32:
//  * chip_features_k    — a striped, soft-binned joint colour histogram per chip: features [capacity][64 stripes];
//  * feature_overlap_k  — histogram intersection of every chip with every track: S[k][t] = sum_d min(F[k][d], G[t][d]),
//                         a tiled (min, +) product;
//  * track_features_k   — the descriptor of the chip that matched or started a track copied or blended into the track's.
// ops/image.py's chip_features, feature_overlap and track_update state the rules in full.
//
// chip_features_k. One workgroup of 256 threads per (stripe, slot): the grid depends on (stripes, capacity) alone, so a
// captured graph replays it. A stripe is a run of whole chip rows, so its bytes are one contiguous span of the chips
// tensor, at any alignment (S_w * 3 is no multiple of 4 in general). Thread g takes 4 pixels = 12 bytes a trip through
// load_bytes of image_stage.h: aligned dwords where the span holds all four of their bytes, single bytes at the span's
// two ends, nothing outside it. A slot whose row is negative stores zeros and returns before it has read a byte.
//  Histogram. A stripe has 64 joint bins. LDS holds FEAT_COPIES = 64 copies of them, one per *lane*, shared by the
//  workgroup's four waves: word bin * FEAT_STRIDE + lane with FEAT_STRIDE = 65. The reasons:
//   - No two lanes of one instruction ever touch the same word, whatever the picture: a flat-coloured region, where
//     every lane votes into the same bin, becomes 64 consecutive words — one per bank, no conflict and no same-address
//     serialisation, which is what copies per wave or per quarter-wave (4 to 64 lanes on one word) would still have.
//     Only the four waves meet on a word, so the update stays an LDS atomic (ds_add_u32 without return).
//   - With the odd stride a random picture spreads as well: lane l voting into bin b lands in bank (b + l) mod 64.
//     The eight votes of one lane are eight instructions, so they never compete with each other for a bank.
//   - 64 x 65 words are 16.3 KB: 9 workgroups a CU by LDS, and the 8 that 256 threads allow bind first. Copies per
//     wave *and* lane (4 x as much) would leave 2 workgroups a CU and save only the atomic's cross-wave arbitration.
//   - Two cheaper remedies for flat regions come before the LDS: a thread merges a run of equal pixels among its four
//     into one set of votes with the weights times the run length, and a vote of weight zero is not cast (a channel
//     value on a bin centre has one bin, so a flat pixel on centres casts 1 vote, not 8).
//  Reduction and store. After a barrier thread (bin = tid & 63, q = tid >> 6) sums copies 16 q .. 16 q + 15 of its bin
//  — lanes read consecutive bins at stride 65, one bank each — the four partial sums meet in LDS, and threads 0..63
//  store the stripe's 64 consecutive int32: one 256-byte segment.
//
// feature_overlap_k. Tiles of OV_TK = 32 chips x OV_TT = 64 tracks per workgroup of 256 threads, D streamed through
// LDS in chunks of OV_D = 64 (D = 64 stripes, so there is no ragged chunk). Thread (ty, tx) of 16 x 16 holds a 2 x 4
// register micro-tile, chips ty + 16 i and tracks tx + 16 j: strided, so that the 16 tx of a row read 16 consecutive
// LDS rows. LDS rows are OV_D + 1 = 65 words: a wave's 16 track rows start in 16 different banks and its 4 chip rows
// are broadcasts. Per step of d a thread reads 6 words for 8 min-adds. 2 x 4 and not 4 x 4: the largest matrix
// (256 x 1024) is then 128 workgroups instead of 64 on a GPU of 256 CUs, and the problem is bound by launch latency
// long before the LDS ratio matters. The next chunk's global reads (int4, 6 a thread) are issued into registers before
// the current chunk is summed. Rows past capacity or T are zeros in LDS and never stored; S is written in full.
// The matrix cores do not apply: min is not a product, and exactness in 32 bits rules out encoding it as one.
//
// track_features_k. One workgroup of 128 threads per track slot: has[t] is read by all threads before a barrier and
// written by thread 0 behind it, so no element of the slot sees the new flag.
//
// What the compiler reports (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): chip_features_k 17664 bytes of
// LDS (the copies and the 1 KB of partial sums), 30 VGPRs, 8 waves a SIMD; feature_overlap_k 24960 bytes, 102 VGPRs
// (the micro-tile, the six int4 in flight and the d loop unrolled by 8), 4 waves a SIMD; track_features_k no LDS, 20
// VGPRs; nothing spilled to scratch.
// Not measured: 64 shared copies against per-wave or fewer copies, FEAT_STRIDE 65 against other odd strides, the run
// merge on and off, 32 x 64 tiles and the 2 x 4 micro-tile against 64 x 64 / 4 x 4, b32 against b128 LDS reads, and
// LDS bank-conflict counters for any of it: the bank arguments above are arithmetic.
// Included by image.hip alone, after image_stage.h (load_bytes).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "image_stage.h"

namespace {
constexpr int FT = 256, FEAT_BINS = 64, FEAT_COPIES = 64, FEAT_STRIDE = FEAT_COPIES + 1;
constexpr int FEAT_MAX_STRIPES = 8, FEAT_MAX_D = FEAT_BINS * FEAT_MAX_STRIPES, FEAT_MAX_SHIFT = 8;
constexpr int OV_TK = 32, OV_TT = 64, OV_D = 64, OV_ROW = OV_D + 1, OV_MAX_K = 256, OV_MAX_T = 1024;
static_assert(FEAT_STRIDE % 2 == 1 && FEAT_COPIES == 64 && FT == 4 * FEAT_BINS, "a copy per lane; 4 partial sums a bin");
static_assert(OV_TK * OV_D / 4 == 2 * FT && OV_TT * OV_D / 4 == 4 * FT && FT == 256, "2 + 4 int4 a thread and chunk");

// one channel value: its lower bin k and the weight f of the bin above (16 - f stays with k)
__device__ __forceinline__ void feat_channel(uint32_t v, int& k, int& f) {
  const int p = min(max(int(v) - 32, 0), 192);
  k = p >> 6, f = (p & 63) >> 2;
}

// pixel px (R | G << 8 | B << 16) seen n times: up to 8 votes, n * 4096 in all, into the lane's copy
__device__ __forceinline__ void feat_vote(uint32_t* hist, uint32_t px, uint32_t n) {
  int kr, fr, kg, fg, kb, fb;
  feat_channel(px & 255, kr, fr), feat_channel(px >> 8 & 255, kg, fg), feat_channel(px >> 16 & 255, kb, fb);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int ur = c >> 2, ug = c >> 1 & 1, ub = c & 1;
    const uint32_t w = uint32_t((ur ? fr : 16 - fr) * (ug ? fg : 16 - fg) * (ub ? fb : 16 - fb));
    // a weight above the last bin is zero (p = 192 has f = 0), so k + 1 never passes 3 here
    if (w) atomicAdd(hist + (((kr + ur) * 4 + kg + ug) * 4 + kb + ub) * FEAT_STRIDE, w * n);
  }
}

// chips [capacity][sh][sw][3] uint8, rows [capacity] -> features [capacity][64 stripes] int32; grid (stripes, capacity)
__global__ __launch_bounds__(FT) void chip_features_k(const uint8_t* __restrict__ chips, const int* __restrict__ rows,
                                                      int sh, int sw, int stripes, int* __restrict__ features) {
  __shared__ uint32_t s_hist[FEAT_BINS * FEAT_STRIDE];
  __shared__ uint32_t s_part[FT / FEAT_BINS][FEAT_BINS];
  const int tid = threadIdx.x, lane = tid & 63, s = blockIdx.x, slot = blockIdx.y;
  int* const out = features + (size_t(slot) * stripes + s) * FEAT_BINS;
  if (rows[slot] < 0) {  // the same in every thread
    if (tid < FEAT_BINS) out[tid] = 0;
    return;
  }
  for (int e = tid; e < FEAT_BINS * FEAT_STRIDE; e += FT) s_hist[e] = 0;
  __syncthreads();
  const int r0 = s * sh / stripes, r1 = (s + 1) * sh / stripes, npix = (r1 - r0) * sw;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(chips) + (size_t(slot) * sh + r0) * sw * 3, hi = lo + size_t(npix) * 3;
  uint32_t* const hist = s_hist + lane;
  for (int g = tid * 4; g < npix; g += FT * 4) {
    uint32_t w[3];
    load_bytes<12>(w, lo + size_t(g) * 3, lo, hi);
    const uint32_t px[4] = {w[0] & 0xffffffu, (w[0] >> 24 | w[1] << 8) & 0xffffffu, (w[1] >> 16 | w[2] << 16) & 0xffffffu,
                            w[2] >> 8};
    const int n = min(4, npix - g);
    uint32_t run = 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= n) break;
      if (j + 1 < n && px[j + 1] == px[j]) {
        ++run;
        continue;
      }
      feat_vote(hist, px[j], run);
      run = 1;
    }
  }
  __syncthreads();
  const int bin = tid & 63, q = tid >> 6;
  uint32_t sum = 0;
#pragma unroll
  for (int c = 0; c < FEAT_COPIES / 4; ++c) sum += s_hist[bin * FEAT_STRIDE + q * (FEAT_COPIES / 4) + c];
  s_part[q][bin] = sum;
  __syncthreads();
  if (tid < FEAT_BINS) out[tid] = int(s_part[0][tid] + s_part[1][tid] + s_part[2][tid] + s_part[3][tid]);
}

// Rows r0 + (e >> 4) (e = tid + FT i), int4 number e & 15 of chunk d0 of a [n][D] matrix, zeros past its last row.
template <int NV>
__device__ __forceinline__ void overlap_fetch(int4 (&v)[NV], const int* __restrict__ m, int n, int D, int r0, int d0,
                                              int tid) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int e = tid + FT * i, r = r0 + (e >> 4);
    v[i] = r < n ? *reinterpret_cast<const int4*>(m + size_t(r) * D + d0 + (e & 15) * 4) : make_int4(0, 0, 0, 0);
  }
}

template <int NV>
__device__ __forceinline__ void overlap_stage(int* s, const int4 (&v)[NV], int tid) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int e = tid + FT * i;
    int* const p = s + (e >> 4) * OV_ROW + (e & 15) * 4;
    p[0] = v[i].x, p[1] = v[i].y, p[2] = v[i].z, p[3] = v[i].w;
  }
}

// F [K][D], G [T][D] int32 (16-byte aligned, D a multiple of 64) -> S [K][T]; grid (ceil(T / 64), ceil(K / 32))
__global__ __launch_bounds__(FT) void feature_overlap_k(const int* __restrict__ F, const int* __restrict__ G, int K, int T,
                                                        int D, int* __restrict__ S) {
  __shared__ int s_f[OV_TK * OV_ROW], s_g[OV_TT * OV_ROW];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int k0 = int(blockIdx.y) * OV_TK, t0 = int(blockIdx.x) * OV_TT;
  int acc[2][4] = {};
  int4 vf[2], vg[4];
  overlap_fetch(vf, F, K, D, k0, 0, tid);
  overlap_fetch(vg, G, T, D, t0, 0, tid);
  for (int d0 = 0; d0 < D; d0 += OV_D) {  // D is the same in every thread: the barriers are the workgroup's
    overlap_stage(s_f, vf, tid);
    overlap_stage(s_g, vg, tid);
    __syncthreads();
    if (d0 + OV_D < D) {
      overlap_fetch(vf, F, K, D, k0, d0 + OV_D, tid);
      overlap_fetch(vg, G, T, D, t0, d0 + OV_D, tid);
    }
#pragma unroll 8
    for (int d = 0; d < OV_D; ++d) {
      int a[2], b[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = s_f[(ty + 16 * i) * OV_ROW + d];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = s_g[(tx + 16 * j) * OV_ROW + d];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += min(a[i], b[j]);
    }
    __syncthreads();  // the chunk is summed, and the tiles are free for the next one
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + ty + 16 * i, t = t0 + tx + 16 * j;
      if (k < K && t < T) S[size_t(k) * T + t] = acc[i][j];
    }
}

// features [K][D] (this frame's chips), the state's ids / src [T] as the tracker variant left them, feat [T][D],
// has [T]: a free slot is zeroed, a slot with a source copies (has == 0 or shift == 0) or blends its descriptor:
// old + floor((new - old + 2^(shift - 1)) / 2^shift). Grid T, 128 threads.
__global__ __launch_bounds__(128) void track_features_k(const int* __restrict__ features, int K, int D,
                                                        const int* __restrict__ ids, const int* __restrict__ src,
                                                        int* __restrict__ feat, int* __restrict__ has, int shift) {
  const int t = blockIdx.x, tid = threadIdx.x;
  const int id = ids[t], k = src[t], had = has[t];  // the same in every thread
  int* const mine = feat + size_t(t) * D;
  if (id == 0) {
    for (int d = tid; d < D; d += 128) mine[d] = 0;
    if (tid == 0) has[t] = 0;
    return;
  }
  if (k < 0 || k >= K) return;
  const int* const chip = features + size_t(k) * D;
  const int half = shift > 0 ? 1 << (shift - 1) : 0;
  for (int d = tid; d < D; d += 128) {
    const int nw = chip[d], old = mine[d];
    mine[d] = had != 0 && shift > 0 ? old + ((nw - old + half) >> shift) : nw;
  }
  __syncthreads();  // every thread has read has[t]
  if (tid == 0) has[t] = 1;
}
}  // namespace
