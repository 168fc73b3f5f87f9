// nos x3 GEMM for gfx950: fp32-accurate C = A · W^T on the bf16 matrix cores.
//
// Every fp32 operand arrives as three bf16 planes (x = x0 + x1 + x2 exactly; see kernels.hip
// "fp32 as three bf16 planes"): activations are split by their producer (LayerNorm, attention,
// the previous GEMM's epilogue), weights once at load time. Each 32x32x16 block is six
// v_mfma_f32_32x32x16_bf16 (a2b0, a1b1, a0b2, a1b0, a0b1, a0b0 — small terms first) = 192
// matrix-pipe cycles against 512 for the same block on v_mfma_f32_32x32x2_f32, with the dropped
// products (a1b2, a2b1, a2b2) at 2^-24 relative: fp32 accuracy at 2.67x the f32 MFMA rate.
//
//  * four waves in a 2x2 grid, each owning a WM x WN sub-tile (1-4 32x32 accumulators); stages of
//    BK = 32 (two MFMA k-steps) per plane;
//  * LDS images [plane][row][40] bf16: a lane's fragment A[row j][16s + 8h .. +7] is one
//    ds_read_b128; the 80-B row stride maps the rows of every ds_read_b128 lane group to distinct
//    16-B bank slots (5r mod 16 is a bijection), so reads are conflict-free;
//  * double-buffered (or single-buffered for twice the resident workgroups) with the next stage's
//    16-B global loads held in registers across the MFMAs; XCD-major tile order;
//  * fused epilogue: bias, exact GELU, residual, broadcast second residual; the result goes out
//    as fp32 and/or as three bf16 planes (split in registers) for the next x3 consumer.
//
// That is gemm_x3, the register-staged kernel. The other five families take their operand tiles
// global -> LDS by DMA (x3_dma.h: the swizzled LDS image, the waits, one stage's DMA and the S-stage
// ring X3_RING) and share the epilogue:
//  * gemm_x3d: one tile (or one K split of it) per workgroup through the ring, on 32x32x16 or
//    16x16x32 MFMAs;
//  * gemm_x3s: persistent; a workgroup's tiles are one stage stream through the ring;
//  * gemm_x3k: stream-K partials; a workgroup's share of all K stages is one stream through the ring;
//  * gemm_x3t: 8 waves on 16x16x32, half of them half a stage behind (its own three-buffer loop);
//  * gemm_x3a: fp32 A split into planes in the kernel (its own loop, register-staged A, DMA for W).
// Host side: every entry point fills one X3Args, every launch goes through launch(), and each
// family's configurations are listed once, in kTiles / kPersistent / kStreamK / kF32A.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "epilogue.h"
#include "pin.h"
#include "streamk.h"
#include "x3_common.h"
#include "x3_dma.h"
#include "x3_schedule.h"

namespace {
thread_local std::string g_err;

enum : int { EPI_NONE = 0, EPI_BIAS = 1, EPI_GELU = 2, EPI_RES = 4, EPI_RES2 = 8 };
constexpr int BK = 32, LSTR = 40;

__device__ __forceinline__ int acc_row(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

// rows x 32 bf16 per plane = rows*4 16-B chunks; chunk f = tid + 256*v -> row f/4, k offset 8*(f%4)
template <int ROWS>
struct Tile {
  static constexpr int V = ROWS * 4 / 256;  // chunks per thread per plane
};

template <int ROWS>
__device__ __forceinline__ void fetch(uint4 (&r)[3][Tile<ROWS>::V], const __bf16* __restrict__ X, size_t plane,
                                      int r0, int rmax, int K, int k0, int tid) {
#pragma unroll
  for (int v = 0; v < Tile<ROWS>::V; ++v) {
    const int f = tid + 256 * v, row = min(r0 + (f >> 2), rmax);
    const __bf16* p = X + size_t(row) * K + k0 + 8 * (f & 3);
#pragma unroll
    for (int q = 0; q < 3; ++q) r[q][v] = *reinterpret_cast<const uint4*>(p + q * plane);
  }
}

template <int ROWS>
__device__ __forceinline__ void stash(const uint4 (&r)[3][Tile<ROWS>::V], __bf16* s, int tid) {
#pragma unroll
  for (int v = 0; v < Tile<ROWS>::V; ++v) {
    const int f = tid + 256 * v;
#pragma unroll
    for (int q = 0; q < 3; ++q)
      *reinterpret_cast<uint4*>(s + q * ROWS * LSTR + (f >> 2) * LSTR + 8 * (f & 3)) = r[q][v];
  }
}

template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void compute_stage(f32x16 (&acc)[WM / 32][WN / 32], const __bf16* __restrict__ as,
                                              const __bf16* __restrict__ bs, int wm, int wn, int j, int hf) {
  constexpr int TM = WM / 32, TN = WN / 32;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bf16x8 af[TM][3], bfr[TN][3];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int q = 0; q < 3; ++q)
        af[a][q] = *reinterpret_cast<const bf16x8*>(&as[q * BM * LSTR + (wm * WM + 32 * a + j) * LSTR + 16 * s + 8 * hf]);
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int q = 0; q < 3; ++q)
        bfr[b][q] = *reinterpret_cast<const bf16x8*>(&bs[q * BN * LSTR + (wn * WN + 32 * b + j) * LSTR + 16 * s + 8 * hf]);
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b)
        acc[a][b] = mfma_x3(af[a][0], af[a][1], af[a][2], bfr[b][0], bfr[b][1], bfr[b][2], acc[a][b]);
  }
}

// two values of one column in adjacent rows (idx, idx + N): the plane split on packed pairs
__device__ __forceinline__ void store_pair(float v0, float v1, size_t idx, int N, float* __restrict__ C,
                                           __bf16* __restrict__ Cp, size_t c_plane) {
  if (C) C[idx] = v0, C[idx + N] = v1;
  if (Cp) {
    nos_bf2 pl[3];
    nos_split3_pair(nos_f2{v0, v1}, pl);
#pragma unroll
    for (int q = 0; q < 3; ++q) Cp[q * c_plane + idx] = pl[q].x, Cp[q * c_plane + idx + N] = pl[q].y;
  }
}

__device__ __forceinline__ void store_one(float v, size_t idx, float* __restrict__ C, __bf16* __restrict__ Cp,
                                          size_t c_plane) {
  if (C) C[idx] = v;
  if (Cp) {
    const __bf16 h0 = (__bf16)v;
    const float r1 = v - (float)h0;
    const __bf16 h1 = (__bf16)r1;
    Cp[idx] = h0;
    Cp[c_plane + idx] = h1;
    Cp[2 * c_plane + idx] = (__bf16)(r1 - (float)h1);
  }
}

// Epilogue math of one 32x32 accumulator: bias, GELU, residuals (the API order). Operands are loaded for all 16
// rows at once, from clamped (always valid) rows: a per-element "if (row < M) load" becomes a
// branch and a vmcnt(0) per element (16 dependent memory round trips per accumulator).
__device__ __forceinline__ void epi_values(const f32x16& acc, float (&v)[16], int rb, int col, int hf, float bv,
                                           const float* __restrict__ R, const float* __restrict__ R2, int r2_rows,
                                           int M, int N, int epi) {
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = acc[r] + bv;
  if (epi & EPI_GELU) {
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const nos_f2 g = nos_gelu2(nos_f2{v[r], v[r + 1]});
      v[r] = g.x, v[r + 1] = g.y;
    }
  }
  if (epi & EPI_RES) {
    float rv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rv[r] = R[size_t(min(rb + acc_row(r, hf), M - 1)) * N + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] += rv[r];
  }
  if (epi & EPI_RES2) {
    float rv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rv[r] = R2[size_t(min(rb + acc_row(r, hf), M - 1) % r2_rows) * N + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] += rv[r];
  }
}

// Fused epilogue of a wave's TM x TN accumulators at rows r0.., columns c0..: register r of
// acc[a][b] is C[r0 + 32a + acc_row(r, hf)][c0 + 32b + j]; bias, exact GELU, residuals; fp32 and/or
// x3 planes out.
template <int TM, int TN>
__device__ __forceinline__ void store_tile(const f32x16 (&acc)[TM][TN], int r0, int c0, int j, int hf,
                                           const float* __restrict__ bias, const float* __restrict__ R,
                                           const float* __restrict__ R2, int r2_rows, float* __restrict__ C,
                                           __bf16* __restrict__ Cp, size_t c_plane, int M, int N, int epi) {
#pragma unroll
  for (int b = 0; b < TN; ++b) {
    const int col = c0 + 32 * b + j;
    const float bv = (epi & EPI_BIAS) ? bias[col] : 0.f;
#pragma unroll
    for (int a = 0; a < TM; ++a) {
      float v[16];
      epi_values(acc[a][b], v, r0 + 32 * a, col, hf, bv, R, R2, r2_rows, M, N, epi);
      // full 32-row blocks (all but the last row of tiles) store without per-element predicates
      if (r0 + 32 * a + 32 <= M) {
        // registers r, r+1 (r even) are rows acc_row(r) and acc_row(r) + 1
#pragma unroll
        for (int r = 0; r < 16; r += 2)
          store_pair(v[r], v[r + 1], size_t(r0 + 32 * a + acc_row(r, hf)) * N + col, N, C, Cp, c_plane);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = r0 + 32 * a + acc_row(r, hf);
          if (row < M) store_one(v[r], size_t(row) * N + col, C, Cp, c_plane);
        }
      }
    }
  }
}

template <int WM, int WN, int NBUF>
__global__ __launch_bounds__(256, 2) void gemm_x3(const __bf16* __restrict__ A, size_t a_plane,
                                                 const __bf16* __restrict__ W, size_t w_plane,
                                                 const float* __restrict__ bias, const float* __restrict__ R,
                                                 const float* __restrict__ R2, int r2_rows, float* __restrict__ C,
                                                 __bf16* __restrict__ Cp, size_t c_plane, int M, int N, int K,
                                                 int epi) {
  constexpr int BM = 2 * WM, BN = 2 * WN;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int VA = Tile<BM>::V, VB = Tile<BN>::V;
  __shared__ __attribute__((aligned(16))) __bf16 As[NBUF][3 * BM * LSTR];
  __shared__ __attribute__((aligned(16))) __bf16 Bs[NBUF][3 * BN * LSTR];

  const int group = (epi >> 8) & 0xff;
  const PinnedBlock pb = pinned_block(unsigned(epi >> 20) & 0xffu);
  epi &= 0xff;
  if (pb.id < 0) return;
  const int tiles_n = N / BN, tiles_m = (M + BM - 1) / BM;
  int t, sp, mt, nt;
  if (!x3_unit(pb.id, pb.n, pb.nx, tiles_m * tiles_n, 1, t, sp)) return;
  tile_rc(t, tiles_m, tiles_n, group, mt, nt);
  const int m0 = mt * BM, n0 = nt * BN;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int j = lane & 31, hf = lane >> 5;

  uint4 pa0[3][VA], pb0[3][VB];
  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b) acc[a][b] = f32x16{0};

  const int nk = K / BK;
// past the end a load re-reads the last stage: loads stay unconditional, so the prefetch registers
// are never conditionally live (the compiler would demote them to scratch)
#define X3_LOAD(RA, RB, STAGE)                                           \
  {                                                                      \
    const int k0_ = min((STAGE), nk - 1) * BK;                           \
    fetch<BM>(RA, A, a_plane, m0, M - 1, K, k0_, tid);                   \
    fetch<BN>(RB, W, w_plane, n0, N - 1, K, k0_, tid);                   \
  }
#define X3_PUT(RA, RB, BUF)                                              \
  {                                                                      \
    if constexpr (NBUF == 1) {                                           \
      __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0) */               \
      __builtin_amdgcn_s_barrier();                                      \
    }                                                                    \
    stash<BM>(RA, As[BUF], tid);                                         \
    stash<BN>(RB, Bs[BUF], tid);                                         \
    __syncthreads();                                                     \
  }
// one stage ks: stage ks+1 is loaded into (NA, NB) across the MFMAs of stage ks, then stashed
#define X3_STEP(KS, NA, NB)                                              \
  {                                                                      \
    const int buf_ = NBUF == 2 ? ((KS) & 1) : 0;                         \
    X3_LOAD(NA, NB, (KS) + 1)                                            \
    compute_stage<BM, BN, WM, WN>(acc, As[buf_], Bs[buf_], wm, wn, j, hf); \
    X3_PUT(NA, NB, NBUF == 2 ? (buf_ ^ 1) : 0)                           \
  }

  X3_LOAD(pa0, pb0, 0)
  X3_PUT(pa0, pb0, 0)
  for (int ks = 0; ks < nk; ++ks) X3_STEP(ks, pa0, pb0)
#undef X3_STEP
#undef X3_PUT
#undef X3_LOAD

  // epilogue: acc[a][b] register r is C[m0 + wm*WM + 32a + acc_row(r, hf)][n0 + wn*WN + 32b + j]
  store_tile<TM, TN>(acc, m0 + wm * WM, n0 + wn * WN, j, hf, bias, R, R2, r2_rows, C, Cp, c_plane, M, N, epi);
}

// ---- LDS-DMA variant ---------------------------------------------------------------------------
// Same math and epilogue; the operand tiles go global -> LDS by DMA (x3_dma.h: the LDS image, the
// waits and the S-stage ring).
template <int BM, int BN, int WM, int WN, int BKS = 32>
__device__ __forceinline__ void compute_stage_sw(f32x16 (&acc)[WM / 32][WN / 32], const __bf16* __restrict__ as,
                                                 const __bf16* __restrict__ bs, int wm, int wn, int j, int hf) {
  constexpr int TM = WM / 32, TN = WN / 32;
  const int sw = dma_swz<BKS>(j);  // rows j and j + 32a share the swizzle
#pragma unroll
  for (int s = 0; s < BKS / 16; ++s) {
    const int ch = (2 * s + hf) ^ sw;
    bf16x8 af[TM][3], bfr[TN][3];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int q = 0; q < 3; ++q)
        af[a][q] = *reinterpret_cast<const bf16x8*>(&as[q * BM * BKS + (wm * WM + 32 * a + j) * BKS + 8 * ch]);
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int q = 0; q < 3; ++q)
        bfr[b][q] = *reinterpret_cast<const bf16x8*>(&bs[q * BN * BKS + (wn * WN + 32 * b + j) * BKS + 8 * ch]);
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b)
        acc[a][b] = mfma_x3(af[a][0], af[a][1], af[a][2], bfr[b][0], bfr[b][1], bfr[b][2], acc[a][b]);
  }
}

// ---- 16x16x32 variant --------------------------------------------------------------------------
// The same x3 product on v_mfma_f32_16x16x32_bf16: equal matrix-pipe cycles per FLOP, and on random
// data the smaller shape holds a higher clock when the whole chip is power-limited (the concurrent
// partitions of the bench). Fragment: lane l = row l%16, k 8(l/16)..+7 of a 32-deep stage; result:
// lane l = column l%16, rows 4(l/16)..+3 of a 16x16 block.
__device__ __forceinline__ f32x4 mfma_x3_16(const bf16x8& a0, const bf16x8& a1, const bf16x8& a2, const bf16x8& b0,
                                            const bf16x8& b1, const bf16x8& b2, f32x4 d) {
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b0, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b2, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, d, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, d, 0, 0, 0);
}

template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void compute_stage16(f32x4 (&acc)[WM / 16][WN / 16], const __bf16* __restrict__ as,
                                                const __bf16* __restrict__ bs, int wm, int wn, int lane) {
  constexpr int TM = WM / 16, TN = WN / 16;
  const int r16 = lane & 15;
  const int ch = (lane >> 4) ^ dma_swz<32, true>(r16);  // rows r16 + 16a share the swizzle
  bf16x8 af[TM][3], bfr[TN][3];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int q = 0; q < 3; ++q)
      af[a][q] = *reinterpret_cast<const bf16x8*>(&as[q * BM * 32 + (wm * WM + 16 * a + r16) * 32 + 8 * ch]);
#pragma unroll
  for (int b = 0; b < TN; ++b)
#pragma unroll
    for (int q = 0; q < 3; ++q)
      bfr[b][q] = *reinterpret_cast<const bf16x8*>(&bs[q * BN * 32 + (wn * WN + 16 * b + r16) * 32 + 8 * ch]);
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
      acc[a][b] = mfma_x3_16(af[a][0], af[a][1], af[a][2], bfr[b][0], bfr[b][1], bfr[b][2], acc[a][b]);
}

template <int TM, int TN>
__device__ __forceinline__ void store_tile16(const f32x4 (&acc)[TM][TN], int r0, int c0, int lane,
                                             const float* __restrict__ bias, const float* __restrict__ R,
                                             const float* __restrict__ R2, int r2_rows, float* __restrict__ C,
                                             __bf16* __restrict__ Cp, size_t c_plane, int M, int N, int epi) {
  const int cl = lane & 15, rq = 4 * (lane >> 4);
#pragma unroll
  for (int b = 0; b < TN; ++b) {
    const int col = c0 + 16 * b + cl;
    const float bv = (epi & EPI_BIAS) ? bias[col] : 0.f;
#pragma unroll
    for (int a = 0; a < TM; ++a) {
      const int rb = r0 + 16 * a + rq;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = acc[a][b][i] + bv;
      if (epi & EPI_GELU) {
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
          const nos_f2 g = nos_gelu2(nos_f2{v[i], v[i + 1]});
          v[i] = g.x, v[i + 1] = g.y;
        }
      }
      if (epi & EPI_RES) {
        float rv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) rv[i] = R[size_t(min(rb + i, M - 1)) * N + col];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] += rv[i];
      }
      if (epi & EPI_RES2) {
        float rv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) rv[i] = R2[size_t(min(rb + i, M - 1) % r2_rows) * N + col];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] += rv[i];
      }
      if (rb + 4 <= M) {
#pragma unroll
        for (int i = 0; i < 4; i += 2) store_pair(v[i], v[i + 1], size_t(rb + i) * N + col, N, C, Cp, c_plane);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (rb + i < M) store_one(v[i], size_t(rb + i) * N + col, C, Cp, c_plane);
      }
    }
  }
}

// BM x BN tile on a WGM x WGN grid of waves (4 or 8 waves: 8 gives each SIMD two waves of one
// workgroup, so a 128x128 tile — half the bytes per MFMA of 64x64 — still hides its load latency)
template <int BM, int BN, int WGM, int WGN, int S, int BKS = 32, bool M16 = false>
__global__ __launch_bounds__(64 * WGM * WGN, 1) void gemm_x3d(const __bf16* __restrict__ A, size_t a_plane,
                                                  const __bf16* __restrict__ W, size_t w_plane,
                                                  const float* __restrict__ bias, const float* __restrict__ R,
                                                  const float* __restrict__ R2, int r2_rows, float* __restrict__ C,
                                                  __bf16* __restrict__ Cp, size_t c_plane, int M, int N, int K,
                                                  int epi) {
  using G = X3Waves<BM, BN, WGM, WGN, BKS>;
  constexpr int NW = G::NW, WM = G::WM, WN = G::WN;
  static_assert(!M16 || BKS == 32, "16x16x32 tiles use 32-deep stages");
  X3_STAGE_BUFFERS(S, BM, BN, BKS);

  const int group = (epi >> 8) & 0xff, ablate = (epi >> 16) & 7, splits = 1 + ((epi >> 28) & 7);
  const PinnedBlock pb = pinned_block(unsigned(epi >> 20) & 0xffu);
  epi &= 0xff;
  if (pb.id < 0) return;
  const int tiles_n = N / BN, tiles_m = (M + BM - 1) / BM;
  // split-K partials (splits > 1): unit = (tile, split), a tile's splits adjacent (one XCD's L2);
  // split sp sums K stages [sp*nk/splits, (sp+1)*nk/splits) into fp32 plane sp of C [splits][M][N]
  // with no epilogue — the consumer (splitk_layernorm) adds the planes, bias and residuals
  int t, sp, mt, nt;
  if (!x3_unit(pb.id, pb.n, pb.nx, tiles_m * tiles_n, splits, t, sp)) return;
  if (splits > 1) C += size_t(sp) * M * N;
  tile_rc(t, tiles_m, tiles_n, group, mt, nt);
  const int m0 = mt * BM, n0 = nt * BN;

  X3_WAVE_LOCALS(WGN);
  f32x16 acc[M16 ? 1 : G::TM][M16 ? 1 : G::TN];
  f32x4 acc16[M16 ? G::TM16 : 1][M16 ? G::TN16 : 1];
  X3_ZERO_ACC(acc, M16 ? 1 : G::TM, M16 ? 1 : G::TN, f32x16)
  X3_ZERO_ACC(acc16, M16 ? G::TM16 : 1, M16 ? G::TN16 : 1, f32x4)

  const int nk_all = K / BKS, kb = sp * nk_all / splits;
  const int nk = (sp + 1) * nk_all / splits - kb;
  uint32_t voff_a[G::VA], voff_b[G::VB];
  dma_offsets<BM, NW, BKS, M16>(voff_a, m0, M - 1, K, wave, lane);
  dma_offsets<BN, NW, BKS, M16>(voff_b, n0, N - 1, K, wave, lane);
#define X3D_ISSUE(ST, B)                             \
  {                                                                      \
    const int k0_ = (kb + (ST)) * BKS;               \
    X3_DMA_AB(voff_a, voff_b, k0_, X3_A(B), X3_B(B)) \
  }
#define X3D_CONSUME(KS, B)                                                         \
  {                                                                      \
    if constexpr (M16)                                                             \
      compute_stage16<BM, BN, WM, WN>(acc16, X3_A(B), X3_B(B), wm, wn, lane);      \
    else                                                                           \
      compute_stage_sw<BM, BN, WM, WN, BKS>(acc, X3_A(B), X3_B(B), wm, wn, j, hf); \
  }
  X3_RING(S, G::NLD, nk, X3D_ISSUE, X3D_CONSUME)
#undef X3D_CONSUME
#undef X3D_ISSUE
  // direct stores: each instruction writes whole 64/128-byte row segments of two rows. Wider
  // per-lane vectors were measured: through lane-quad DPP transposes slower; through a dedicated
  // wave-private LDS scratch (16-byte row chunks, 8x fewer store instructions for x3 planes)
  // correct run to run but no faster (qkv 27.6 vs 27.6 us, fc1 47.4 vs 46.3 on the whole GPU):
  // the plane bytes, not the instruction count, set the epilogue's time. (A scratch in the freed
  // stage buffers had given run-to-run differences with several workgroups per CU.)
  if constexpr (M16)
    store_tile16<G::TM16, G::TN16>(acc16, m0 + wm * WM, n0 + wn * WN, lane, bias, R, R2, r2_rows, C, Cp, c_plane,
                                   M, N, epi);
  else if (!(ablate & 4))
    store_tile<G::TM, G::TN>(acc, m0 + wm * WM, n0 + wn * WN, j, hf, bias, R, R2, r2_rows, C, Cp, c_plane, M, N,
                             epi);
}

// Persistent (stream-of-stages) LDS-DMA GEMM: a grid of P workgroups, workgroup w owning tiles
// w, w+P, ...; its (tile, k-stage) pairs form one continuous stage stream, so the DMA ring keeps
// loading the next tile's first stages while the current tile's last MFMAs and its epilogue run —
// the fill/drain every short-K (K = 384: 12 stages) tile otherwise pays once per tile.
template <int BM, int BN, int WGM, int WGN, int S, int BKS = 32>
__global__ __launch_bounds__(64 * WGM * WGN, 1) void gemm_x3s(const __bf16* __restrict__ A, size_t a_plane,
                                                              const __bf16* __restrict__ W, size_t w_plane,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ R,
                                                              const float* __restrict__ R2, int r2_rows,
                                                              float* __restrict__ C, __bf16* __restrict__ Cp,
                                                              size_t c_plane, int M, int N, int K, int epi) {
  using G = X3Waves<BM, BN, WGM, WGN, BKS>;
  constexpr int NW = G::NW, WM = G::WM, WN = G::WN;
  X3_STAGE_BUFFERS(S, BM, BN, BKS);

  const int group = (epi >> 8) & 0xff, ablate = (epi >> 16) & 7;
  const PinnedBlock pb = pinned_block(unsigned(epi >> 20) & 0xffu);
  epi &= 0xff;
  if (pb.id < 0) return;
  const int tiles_n = N / BN, tiles_m = (M + BM - 1) / BM;
  const int tiles = tiles_m * tiles_n;
  int tb, ts, tcount;
  xcd_band(pb.id, pb.n, pb.nx, tiles, tb, ts, tcount);
  if (tcount <= 0) return;
  const int nk = K / BKS;
  const int total = tcount * nk;  // this workgroup's stages

  X3_WAVE_LOCALS(WGN);
  f32x16 acc[G::TM][G::TN];
  X3_ZERO_ACC(acc, G::TM, G::TN, f32x16)
#define X3S_ISSUE(H, B)                                           \
  {                                                                      \
    const int h_ = (H), ti_ = h_ / nk, ks_ = h_ - ti_ * nk;       \
    int mt_, nt_;                                                                         \
    tile_rc(tb + ti_ * ts, tiles_m, tiles_n, group, mt_, nt_);    \
    X3_DMA_AB_AT(mt_ * BM, nt_ * BN, ks_ * BKS, X3_A(B), X3_B(B)) \
  }
// the tile's last stage: its epilogue (under the next tile's DMA), and a fresh accumulator
#define X3S_CONSUME(H, B)                                                                         \
  {                                                                      \
    compute_stage_sw<BM, BN, WM, WN, BKS>(acc, X3_A(B), X3_B(B), wm, wn, j, hf);                  \
    if (((H) + 1) % nk == 0) {                                                                    \
    int mt_, nt_;                                                                         \
      tile_rc(tb + ((H) / nk) * ts, tiles_m, tiles_n, group, mt_, nt_);                           \
      if (!(ablate & 4))                                                                          \
        store_tile<G::TM, G::TN>(acc, mt_ * BM + wm * WM, nt_ * BN + wn * WN, j, hf, bias, R, R2, \
                         r2_rows, C, Cp, c_plane, M, N, epi);                             \
      X3_ZERO_ACC(acc, G::TM, G::TN, f32x16)                                                      \
    }                                                                    \
  }
  X3_RING(S, G::NLD, total, X3S_ISSUE, X3S_CONSUME)
#undef X3S_CONSUME
#undef X3S_ISSUE
}

// ---- staggered 8-wave 16x16x32 tiles -----------------------------------------------------------
// Two waves share each SIMD in a 512-thread workgroup, and with one barrier per stage and the same
// program they run in lockstep: both issue their LDS fragment reads, wait on them and reach the
// barrier together, so neither covers the other's stall (MI355X_MICROARCH.md, "Two waves per SIMD",
// item 9). Here the second half of the workgroup (waves NW/2.., the SIMD partners of the first
// half) runs half a stage behind: in stage ks it finishes the second half of its accumulator rows
// for stage ks-1, then the first half for stage ks, so while one wave of a SIMD waits on its reads
// its partner is in the middle of its MFMAs. A stage buffer is therefore read one stage longer:
// three LDS buffers, one stage of DMA in flight (as the two-buffer tiles). Same math and epilogue
// as gemm_x3d<..., M16>; ``rows [R0, R1)`` of the wave's 16-row blocks per call.
template <int BM, int BN, int WM, int WN, int R0, int R1>
__device__ __forceinline__ void compute_rows16(f32x4 (&acc)[WM / 16][WN / 16], const __bf16* __restrict__ as,
                                               const __bf16* __restrict__ bs, int wm, int wn, int lane) {
  constexpr int TN = WN / 16;
  const int r16 = lane & 15;
  const int ch = (lane >> 4) ^ dma_swz<32, true>(r16);
  bf16x8 af[R1 - R0][3], bfr[TN][3];
#pragma unroll
  for (int a = R0; a < R1; ++a)
#pragma unroll
    for (int q = 0; q < 3; ++q)
      af[a - R0][q] = *reinterpret_cast<const bf16x8*>(&as[q * BM * 32 + (wm * WM + 16 * a + r16) * 32 + 8 * ch]);
#pragma unroll
  for (int b = 0; b < TN; ++b)
#pragma unroll
    for (int q = 0; q < 3; ++q)
      bfr[b][q] = *reinterpret_cast<const bf16x8*>(&bs[q * BN * 32 + (wn * WN + 16 * b + r16) * 32 + 8 * ch]);
#pragma unroll
  for (int a = R0; a < R1; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
      acc[a][b] = mfma_x3_16(af[a - R0][0], af[a - R0][1], af[a - R0][2], bfr[b][0], bfr[b][1], bfr[b][2], acc[a][b]);
}

template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(64 * WGM * WGN, 1) void gemm_x3t(const __bf16* __restrict__ A, size_t a_plane,
                                                              const __bf16* __restrict__ W, size_t w_plane,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ R,
                                                              const float* __restrict__ R2, int r2_rows,
                                                              float* __restrict__ C, __bf16* __restrict__ Cp,
                                                              size_t c_plane, int M, int N, int K, int epi) {
  using G = X3Waves<BM, BN, WGM, WGN>;
  constexpr int NW = G::NW, BKS = 32, WM = G::WM, WN = G::WN;
  constexpr int TM16 = G::TM16, TN16 = G::TN16, HM = TM16 / 2;
  static_assert(NW == 8 && TM16 % 2 == 0, "8 waves, an even number of 16-row blocks per wave");
  __shared__ __attribute__((aligned(16))) __bf16 A0[3 * BM * BKS], A1[3 * BM * BKS], A2[3 * BM * BKS];
  __shared__ __attribute__((aligned(16))) __bf16 B0[3 * BN * BKS], B1[3 * BN * BKS], B2[3 * BN * BKS];

  const int group = (epi >> 8) & 0xff, ablate = (epi >> 16) & 7, splits = 1 + ((epi >> 28) & 7);
  const PinnedBlock pb = pinned_block(unsigned(epi >> 20) & 0xffu);
  epi &= 0xff;
  if (pb.id < 0) return;
  const int tiles_n = N / BN, tiles_m = (M + BM - 1) / BM;
  int t, sp, mt, nt;
  if (!x3_unit(pb.id, pb.n, pb.nx, tiles_m * tiles_n, splits, t, sp)) return;
  if (splits > 1) C += size_t(sp) * M * N;
  tile_rc(t, tiles_m, tiles_n, group, mt, nt);
  const int m0 = mt * BM, n0 = nt * BN;

  X3_WAVE_LOCALS(WGN);
  const bool lag = wave >= NW / 2;  // wave-uniform
  f32x4 acc[TM16][TN16];
  X3_ZERO_ACC(acc, TM16, TN16, f32x4)

  const int nk_all = K / BKS, kb = sp * nk_all / splits;
  const int nk = (sp + 1) * nk_all / splits - kb;
  uint32_t voff_a[G::VA], voff_b[G::VB];
  dma_offsets<BM, NW, BKS, true>(voff_a, m0, M - 1, K, wave, lane);
  dma_offsets<BN, NW, BKS, true>(voff_b, n0, N - 1, K, wave, lane);
#define X3T_A(b) X3_BUF(b, A0, A1, A2, A2)
#define X3T_B(b) X3_BUF(b, B0, B1, B2, B2)
#define X3T_ISSUE(STAGE, BUF)                                                      \
  {                                                                      \
    const int k0_ = (kb + (STAGE)) * BKS;                                          \
    X3_DMA_AB(voff_a, voff_b, k0_, X3T_A(BUF), X3T_B(BUF)) \
  }
// stage KS in buffer BUF (= KS % 3): every wave's DMA of it has landed after the wait + barrier, and
// every wave is done with buffer (KS+1) % 3 (read last in stage KS-1 by the lagging half), which
// stage KS+1 then fills
#define X3T_ITER(KS, BUF)                                                          \
  {                                                                      \
    vm_wait<0>();                                                                  \
    raw_barrier();                                                                        \
    if ((KS) + 1 < nk) X3T_ISSUE((KS) + 1, ((BUF) + 1) % 3)                        \
    __builtin_amdgcn_sched_barrier(0);                                             \
    if (!lag) {                                                                    \
      compute_rows16<BM, BN, WM, WN, 0, TM16>(acc, X3T_A(BUF), X3T_B(BUF), wm, wn, lane); \
    } else {                                                                       \
      if ((KS) > 0)                                                                \
        compute_rows16<BM, BN, WM, WN, HM, TM16>(acc, X3T_A(((BUF) + 2) % 3), X3T_B(((BUF) + 2) % 3), wm, wn, lane); \
      compute_rows16<BM, BN, WM, WN, 0, HM>(acc, X3T_A(BUF), X3T_B(BUF), wm, wn, lane); \
    }                                                                    \
  }
  if (nk > 0) X3T_ISSUE(0, 0)
  for (int ks = 0; ks < nk; ks += 3) {
    X3T_ITER(ks, 0)
    if (ks + 1 < nk) X3T_ITER(ks + 1, 1)
    if (ks + 2 < nk) X3T_ITER(ks + 2, 2)
  }
  // the lagging half's last half-stage: no DMA is issued any more, so its buffer is still intact
  if (lag && nk > 0) {
    const int last = (nk - 1) % 3;
    if (last == 0)
      compute_rows16<BM, BN, WM, WN, HM, TM16>(acc, A0, B0, wm, wn, lane);
    else if (last == 1)
      compute_rows16<BM, BN, WM, WN, HM, TM16>(acc, A1, B1, wm, wn, lane);
    else
      compute_rows16<BM, BN, WM, WN, HM, TM16>(acc, A2, B2, wm, wn, lane);
  }
#undef X3T_ITER
#undef X3T_ISSUE
#undef X3T_B
#undef X3T_A
  vm_wait<0>();
  if (!(ablate & 4))
    store_tile16<TM16, TN16>(acc, m0 + wm * WM, n0 + wn * WN, lane, bias, R, R2, r2_rows, C, Cp, c_plane, M, N, epi);
}

// ---- fp32 A operand, split in the kernel -------------------------------------------------------
// The x3 GEMMs are bound by the latency of their operand stream (profiles/pmc_r4_gemm_spx.json:
// waves wait 40-49% of their cycles, the matrix pipe is 16-26% busy). Three bf16 planes are 6 B per
// element where fp32 is 4: here the activation operand arrives as fp32 rows and each thread splits
// its 8-value chunk into the three planes in registers (round to nearest even, the same split the
// producers use, so the planes — and the result — are bit-identical to the planes-in kernel) and
// stores them into the swizzled LDS image the 16x16x32 fragment reads expect. The weight planes
// still come by LDS-DMA. Register-staged A: the next stage's loads are issued before the MFMAs and
// stashed after them, one stage in flight, as the two-buffer tiles.
__device__ __forceinline__ void split3_8(const float4& lo, const float4& hi, bf16x8& a, bf16x8& b, bf16x8& c) {
  split3(f32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}, a, b, c);
}

template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(64 * WGM * WGN, 1) void gemm_x3a(const float* __restrict__ A,
                                                              const __bf16* __restrict__ W, size_t w_plane,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ R,
                                                              const float* __restrict__ R2, int r2_rows,
                                                              float* __restrict__ C, __bf16* __restrict__ Cp,
                                                              size_t c_plane, int M, int N, int K, int epi) {
  using G = X3Waves<BM, BN, WGM, WGN>;
  constexpr int NW = G::NW, BKS = 32, WM = G::WM, WN = G::WN;
  constexpr int TM16 = G::TM16, TN16 = G::TN16;
  constexpr int AC = BM * 4 / (64 * NW);  // 16-B chunks (8 k-values) of the A stage per thread
  static_assert(AC >= 1 && BM * 4 % (64 * NW) == 0, "A stage chunks must divide over the threads");
  __shared__ __attribute__((aligned(16))) __bf16 A0[3 * BM * BKS], A1[3 * BM * BKS];
  __shared__ __attribute__((aligned(16))) __bf16 B0[3 * BN * BKS], B1[3 * BN * BKS];

  const int group = (epi >> 8) & 0xff, ablate = (epi >> 16) & 7, splits = 1 + ((epi >> 28) & 7);
  const PinnedBlock pb = pinned_block(unsigned(epi >> 20) & 0xffu);
  epi &= 0xff;
  if (pb.id < 0) return;
  const int tiles_n = N / BN, tiles_m = (M + BM - 1) / BM;
  int t, sp, mt, nt;
  if (!x3_unit(pb.id, pb.n, pb.nx, tiles_m * tiles_n, splits, t, sp)) return;
  if (splits > 1) C += size_t(sp) * M * N;
  tile_rc(t, tiles_m, tiles_n, group, mt, nt);
  const int m0 = mt * BM, n0 = nt * BN;

  X3_WAVE_LOCALS(WGN);
  f32x4 acc[TM16][TN16];
  X3_ZERO_ACC(acc, TM16, TN16, f32x4)

  const int nk_all = K / BKS, kb = sp * nk_all / splits;
  const int nk = (sp + 1) * nk_all / splits - kb;
  uint32_t voff_b[G::VB];
  dma_offsets<BN, NW, BKS, true>(voff_b, n0, N - 1, K, wave, lane);
  // this thread's A chunks: chunk f = tid + 64*NW*v -> local row f/4, k-chunk f%4; LDS slot
  // (f%4) ^ swz(row), the layout the DMA writes for the 16x16x32 fragment reads
  const float* ap[AC];
  int aoff[AC];
#pragma unroll
  for (int v = 0; v < AC; ++v) {
    const int f = tid + 64 * NW * v, rl = f >> 2, c = f & 3;
    ap[v] = A + size_t(min(m0 + rl, M - 1)) * K + 8 * c;
    aoff[v] = rl * BKS + 8 * (c ^ dma_swz<32, true>(rl));
  }
  float4 ra[AC][2];
#define X3A_A(b) X3_BUF(b, A0, A1, A1, A1)
#define X3A_B(b) X3_BUF(b, B0, B1, B1, B1)
#define X3A_LOAD(STAGE)                                                                 \
  {                                                                      \
    const int k0_ = (kb + (STAGE)) * BKS;                                          \
    if (!(ablate & 2)) dma_stage<BN, NW, BKS>(W, w_plane, voff_b, k0_, X3A_B((STAGE) & 1), wave); \
    _Pragma("unroll") for (int v = 0; v < AC; ++v) {                                    \
      ra[v][0] = *reinterpret_cast<const float4*>(ap[v] + k0_);                         \
      ra[v][1] = *reinterpret_cast<const float4*>(ap[v] + k0_ + 4);                     \
    }                                                                    \
  }
#define X3A_STASH(BUF)                                                                  \
  {                                                                      \
    __bf16* as_ = X3A_A(BUF);                                                           \
    _Pragma("unroll") for (int v = 0; v < AC; ++v) {                                    \
      bf16x8 h0, h1, h2;                                                                \
      split3_8(ra[v][0], ra[v][1], h0, h1, h2);                                         \
      *reinterpret_cast<bf16x8*>(as_ + aoff[v]) = h0;                                   \
      *reinterpret_cast<bf16x8*>(as_ + BM * BKS + aoff[v]) = h1;                        \
      *reinterpret_cast<bf16x8*>(as_ + 2 * BM * BKS + aoff[v]) = h2;                    \
    }                                                                    \
  }
// stage KS in buffer BUF: the barrier publishes every thread's A stash and B DMA of it and frees
// buffer BUF^1 (read in stage KS-1), which stage KS+1 then fills: B by DMA, A loaded into
// registers now and stashed after this stage's MFMAs
#define X3A_ITER(KS, BUF)                                                               \
  {                                                                      \
    vm_wait<0>();                                                                  \
    raw_barrier();                                                                        \
    const bool next_ = (KS) + 1 < nk;                                                   \
    if (next_) X3A_LOAD((KS) + 1)                                                       \
    __builtin_amdgcn_sched_barrier(0);                                             \
    compute_rows16<BM, BN, WM, WN, 0, TM16>(acc, X3A_A(BUF), X3A_B(BUF), wm, wn, lane); \
    if (next_) {                                                                        \
    vm_wait<0>();                                                                  \
      X3A_STASH((BUF) ^ 1)                                                              \
    }                                                                    \
  }
  if (nk > 0) {
    X3A_LOAD(0)
    vm_wait<0>();
    X3A_STASH(0)
  }
  for (int ks = 0; ks < nk; ks += 2) {
    X3A_ITER(ks, 0)
    if (ks + 1 < nk) X3A_ITER(ks + 1, 1)
  }
#undef X3A_ITER
#undef X3A_STASH
#undef X3A_LOAD
#undef X3A_B
#undef X3A_A
  vm_wait<0>();
  if (!(ablate & 4))
    store_tile16<TM16, TN16>(acc, m0 + wm * WM, n0 + wn * WN, lane, bias, R, R2, r2_rows, C, Cp, c_plane, M, N, epi);
}

// ---- stream-K partials -------------------------------------------------------------------------
// The N = 384 GEMMs of the model (projection, fc2) have 162 tiles of 128x64 for 256 CUs: whole-tile
// grids leave a third of the chip idle (or a 27%-full second round), and split-K only moves the
// ragged edge. Here the P workgroups split the tiles' K stages evenly (streamk.h): each runs one
// continuous stage stream as gemm_x3s does (the DMA ring crosses tile boundaries), and at the end
// of every tile segment stores its raw accumulators to fp32 partial plane `segment` — no epilogue;
// the consumer (splitk_layernorm_f32 with the same SkMap) adds a tile's planes in order, then bias,
// residuals and the LayerNorm. The kernel boundary is the hand-off between workgroups (no flags).
template <int BM, int BN, int WGM, int WGN, int S, int BKS = 32>
__global__ __launch_bounds__(64 * WGM * WGN, 1) void gemm_x3k(const __bf16* __restrict__ A, size_t a_plane,
                                                              const __bf16* __restrict__ W, size_t w_plane,
                                                              float* __restrict__ C, int M, int N, int K, int P,
                                                              int ctl) {
  using G = X3Waves<BM, BN, WGM, WGN, BKS>;
  constexpr int NW = G::NW, WM = G::WM, WN = G::WN;
  X3_STAGE_BUFFERS(S, BM, BN, BKS);

  const int ablate = (ctl >> 16) & 7;
  const PinnedBlock pb = pinned_block(unsigned(ctl >> 20) & 0xffu);
  if (pb.id < 0) return;
  const int tiles_n = N / BN, tiles_m = (M + BM - 1) / BM;
  const int nk = K / BKS, U = tiles_m * tiles_n * nk;
  // logical workgroup: XCD x runs a contiguous band of ranges, so the workgroups sharing a tile
  // (neighbouring ranges) mostly share an L2 too
  const int w = xcd_major_n(pb.id, pb.n, pb.nx);
  if (w >= P) return;
  const int u0 = sk_first(w, P, U), total = sk_first(w + 1, P, U) - u0;
  const size_t plane = size_t(M) * N;

  X3_WAVE_LOCALS(WGN);
  f32x16 acc[G::TM][G::TN];
  X3_ZERO_ACC(acc, G::TM, G::TN, f32x16)
#define X3K_ISSUE(H, B)                                           \
  {                                                                      \
    const int u_ = u0 + (H), t_ = u_ / nk, ks_ = u_ - t_ * nk;                            \
    const int mt_ = t_ / tiles_n, nt_ = t_ - mt_ * tiles_n;                               \
    X3_DMA_AB_AT(mt_ * BM, nt_ * BN, ks_ * BKS, X3_A(B), X3_B(B)) \
  }
// a segment ends at its tile's last stage or at the end of this workgroup's range
#define X3K_CONSUME(H, B)                                                                             \
  {                                                                      \
    compute_stage_sw<BM, BN, WM, WN, BKS>(acc, X3_A(B), X3_B(B), wm, wn, j, hf);                      \
    const int u_ = u0 + (H), t_ = u_ / nk;                                                            \
    if (u_ - t_ * nk == nk - 1 || (H) == total - 1) {                                                 \
      const int seg_ = w - sk_owner(t_ * nk, P, U), mt_ = t_ / tiles_n, nt_ = t_ - mt_ * tiles_n; \
      if (!(ablate & 4))                                                                              \
        store_tile<G::TM, G::TN>(acc, mt_ * BM + wm * WM, nt_ * BN + wn * WN, j, hf, nullptr,         \
                                 nullptr, nullptr, 0, C + size_t(seg_) * plane, nullptr, 0, M, N, 0); \
      X3_ZERO_ACC(acc, G::TM, G::TN, f32x16)                                                          \
    }                                                                    \
  }
  X3_RING(S, G::NLD, total, X3K_ISSUE, X3K_CONSUME)
#undef X3K_CONSUME
#undef X3K_ISSUE
}

// ---- host side: one operand struct, one launch path, one table per kernel family ---------------
struct X3Args {
  const void* A;  // three bf16 planes; fp32 rows for gemm_x3a
  size_t ap;
  const __bf16* W;
  size_t wp;
  const float *bias, *R, *R2;
  int r2_rows;
  float* C;
  __bf16* Cp;
  size_t cp;
  int M, N, K;
  int ctl;  // epilogue flags and the control bits of x3_ctl
  int P;    // stream-K workgroups
  hipStream_t s;
};

using KernP = decltype(&gemm_x3<32, 32, 2>);        // planes in, fused epilogue: gemm_x3, x3d, x3s, x3t
using KernA = decltype(&gemm_x3a<128, 128, 2, 4>);  // fp32 A in
using KernK = decltype(&gemm_x3k<64, 64, 2, 2, 3>);  // raw partials out

void enqueue(KernP k, dim3 grid, dim3 block, const X3Args& a) {
  hipLaunchKernelGGL(k, grid, block, 0, a.s, static_cast<const __bf16*>(a.A), a.ap, a.W, a.wp, a.bias, a.R, a.R2,
                     a.r2_rows, a.C, a.Cp, a.cp, a.M, a.N, a.K, a.ctl);
}
void enqueue(KernA k, dim3 grid, dim3 block, const X3Args& a) {
  hipLaunchKernelGGL(k, grid, block, 0, a.s, static_cast<const float*>(a.A), a.W, a.wp, a.bias, a.R, a.R2, a.r2_rows,
                     a.C, a.Cp, a.cp, a.M, a.N, a.K, a.ctl);
}
void enqueue(KernK k, dim3 grid, dim3 block, const X3Args& a) {
  hipLaunchKernelGGL(k, grid, block, 0, a.s, static_cast<const __bf16*>(a.A), a.ap, a.W, a.wp, a.C, a.M, a.N, a.K, a.P,
                     a.ctl);
}

// What a family's messages are prefixed with: a launch error, and the refusals of N and of K
// (n == nullptr: one joint refusal under `err`).
struct Family {
  const char *err, *n, *k;
};
constexpr Family kFamR{"gemm_x3", "gemm_x3", "gemm_x3"}, kFamD{"gemm_x3d", "gemm_x3", "gemm_x3"},
    kFamS{"gemm_x3s", "gemm_x3", "gemm_x3s"}, kFamT{"gemm_x3t", nullptr, nullptr},
    kFamA{"gemm_x3a", nullptr, nullptr}, kFamK{"gemm_x3k", nullptr, nullptr};

// one configuration: BM x BN tile, LDS buffers, stage depth, threads, and its kernel
template <class Kern>
struct Config {
  int bm, bn, nbuf, bks, threads;
  Family fam;
  Kern kern;
};
template <int WM, int WN, int NBUF>
constexpr Config<KernP> reg{2 * WM, 2 * WN, NBUF, BK, 256, kFamR, gemm_x3<WM, WN, NBUF>};
template <int BM, int BN, int WGM, int WGN, int S, int BKS = 32, bool M16 = false>
constexpr Config<KernP> dma{BM, BN, S, BKS, 64 * WGM * WGN, kFamD, gemm_x3d<BM, BN, WGM, WGN, S, BKS, M16>};
template <int BM, int BN, int WGM, int WGN>
constexpr Config<KernP> stag{BM, BN, 3, 32, 64 * WGM * WGN, kFamT, gemm_x3t<BM, BN, WGM, WGN>};
template <int BM, int BN, int WGM, int WGN, int S, int BKS = 32>
constexpr Config<KernP> pers{BM, BN, S, BKS, 64 * WGM * WGN, kFamS, gemm_x3s<BM, BN, WGM, WGN, S, BKS>};
template <int BM, int BN, int WGM, int WGN>
constexpr Config<KernA> f32a{BM, BN, 2, 32, 64 * WGM * WGN, kFamA, gemm_x3a<BM, BN, WGM, WGN>};
template <int BM, int BN, int WGM, int WGN, int S, int BKS = 32>
constexpr Config<KernK> strk{BM, BN, S, BKS, 64 * WGM * WGN, kFamK, gemm_x3k<BM, BN, WGM, WGN, S, BKS>};

// Tile configurations of nos_gemm_x3, id = index. reg<WM, WN, buffers> is the register-staged
// kernel (BM x BN = 2WM x 2WN), dma<BM, BN, WGM, WGN, S, stage depth, 16x16x32> the LDS-DMA pipeline
// with S stage buffers (S-1 stages in flight) on WGM x WGN waves:
constexpr Config<KernP> kTiles[] = {
    // 0-3 = 64x64, 128x64, 64x128, 128x128 (double-buffered LDS)
    reg<32, 32, 2>, reg<64, 32, 2>, reg<32, 64, 2>, reg<64, 64, 2>,
    // 4-6 = 64x64, 128x64, 64x128 (single-buffered: half the LDS, more resident tiles)
    reg<32, 32, 1>, reg<64, 32, 1>, reg<32, 64, 1>,
    // 7-12 = LDS-DMA: 64x64 S3/S4, 128x64 S3, 64x128 S3, 128x128 S3, 64x64 S2
    dma<64, 64, 2, 2, 3>, dma<64, 64, 2, 2, 4>, dma<128, 64, 2, 2, 3>, dma<64, 128, 2, 2, 3>, dma<128, 128, 2, 2, 3>,
    dma<64, 64, 2, 2, 2>,
    // 13/14 = 128x128 on 8 waves S3/S2; 15-17 = 2-wave 32x64 S3/S2, 64x32 S2
    dma<128, 128, 2, 4, 3>, dma<128, 128, 2, 4, 2>, dma<32, 64, 1, 2, 3>, dma<32, 64, 1, 2, 2>, dma<64, 32, 2, 1, 2>,
    // 18-22 = 64-deep stages (128-byte row segments): 64x64 S2/S3, 64x32 S2, 32x64 S2, 64x32 S3
    dma<64, 64, 2, 2, 2, 64>, dma<64, 64, 2, 2, 3, 64>, dma<64, 32, 2, 1, 2, 64>, dma<32, 64, 1, 2, 2, 64>,
    dma<64, 32, 2, 1, 3, 64>,
    // 23/24 = 64-deep on 8 waves: 128x64 S2, 64x128 S2; 25/26 = 128x64 S4, 64x128 S4 (three stages in flight)
    dma<128, 64, 4, 2, 2, 64>, dma<64, 128, 2, 4, 2, 64>, dma<128, 64, 2, 2, 4>, dma<64, 128, 2, 2, 4>,
    // 27-31 = v_mfma 16x16x32: 64x64 S2, 64x64 S3, 128x128 S2 (8 waves), 32x64 S2 (2 waves), 64x32 S2 (2 waves)
    dma<64, 64, 2, 2, 2, 32, true>, dma<64, 64, 2, 2, 3, 32, true>, dma<128, 128, 2, 4, 2, 32, true>,
    dma<32, 64, 1, 2, 2, 32, true>, dma<64, 32, 2, 1, 2, 32, true>,
    // 32-34 = 96/192-wide tiles (three 32-column blocks per wave), so N = 384 / 1536 split into 216
    // tiles at M = 3401 — one round on 256 CUs instead of 1.3-2.5: 128x192 S2, 64x96 S2 (2 waves),
    // 64x192 S2 (2 waves)
    dma<128, 192, 2, 2, 2>, dma<64, 96, 2, 1, 2>, dma<64, 192, 1, 2, 2>,
    // 35-37 = 8 waves of 64x64 each (a third fewer LDS fragment bytes per MFMA than 64x32 waves;
    // 144 KB of LDS for two stages): 256x128 S2, 256x128 S2 on 16x16x32, 128x256 S2
    dma<256, 128, 4, 2, 2>, dma<256, 128, 4, 2, 2, 32, true>, dma<128, 256, 2, 4, 2>,
    // 38 = the staggered 8-wave 16x16x32 128x128 tile (gemm_x3t, three LDS buffers)
    stag<128, 128, 2, 4>};
// nos_gemm_x3_persistent: 0 = 64x64 S3 (4 waves), 1 = 64x64 S2, 2 = 128x128 S3 (8 waves), 3 = 64x128 S3,
// 4 = 128x64 S3; 64-deep stages: 5 = 64x64 S2, 6 = 64x32 S2 (2 waves), 7 = 128x64 S2 (8 waves);
// 8/9 = 128x64, 64x128 S4; 10 = 256x128 S2 (8 waves of 64x64). Tile ids 100.. of nos_gemm_x3_tile.
constexpr Config<KernP> kPersistent[] = {
    pers<64, 64, 2, 2, 3>, pers<64, 64, 2, 2, 2>, pers<128, 128, 2, 4, 3>, pers<64, 128, 2, 2, 3>,
    pers<128, 64, 2, 2, 3>, pers<64, 64, 2, 2, 2, 64>, pers<64, 32, 2, 1, 2, 64>, pers<128, 64, 4, 2, 2, 64>,
    pers<128, 64, 2, 2, 4>, pers<64, 128, 2, 2, 4>, pers<256, 128, 4, 2, 2>};
// nos_gemm_x3_streamk: 0 = 64x64 S3 (4 waves), 1 = 128x64 S2 64-deep (8 waves), 2 = 64x128 S2 64-deep
// (8 waves), 3 = 128x64 S3 (4 waves), 4 = 64x64 S2 64-deep (4 waves), 5 = 128x128 S3 (8 waves)
constexpr Config<KernK> kStreamK[] = {strk<64, 64, 2, 2, 3>,  strk<128, 64, 4, 2, 2, 64>, strk<64, 128, 2, 4, 2, 64>,
                                    strk<128, 64, 2, 2, 3>, strk<64, 64, 2, 2, 2, 64>,  strk<128, 128, 2, 4, 3>};
// nos_gemm_x3_f32a: 0 = 128x128 (8 waves, 16x16x32), 1 = 256x128
constexpr Config<KernA> kF32A[] = {f32a<128, 128, 2, 4>, f32a<256, 128, 4, 2>};
constexpr int kFirstDma = 7, kPersistentBase = 100;  // the first LDS-DMA tile id; tile id of persistent config 0

template <class T, int N>
constexpr int table_size(const T (&)[N]) {
  return N;
}
// entry cfg of a table, or nullptr
template <class T, int N>
const T* pick(const T (&table)[N], int cfg) {
  return cfg >= 0 && cfg < N ? &table[cfg] : nullptr;
}

int refuse(const std::string& why) {
  g_err = why;
  return -1;
}

// units of a one-unit-per-workgroup launch: tiles x K splits (the three bits above the pin mask).
// Only nos_gemm_x3_partials sets split bits, and only for the LDS-DMA tiles: the register-staged and
// persistent kernels do not read them, so an entry point that reaches those must leave them zero.
template <class Kern>
int tile_units(const Config<Kern>& t, const X3Args& a) {
  return ((a.M + t.bm - 1) / t.bm) * (a.N / t.bn) * (1 + ((a.ctl >> 28) & 7));
}

// The one launch: refuses an N or K the tile does not divide, then `units` logical workgroups
// (dealt over the pinned XCDs, pin.h). The register-staged family has no K refusal of its own: its
// stage depth is the K % 32 every entry point refuses first, so the one here cannot fire for it.
template <class Kern>
int launch(const Config<Kern>& t, int units, const X3Args& a) {
  const Family& f = t.fam;
  if (a.N % t.bn || a.K % t.bks) {
    const std::string bn = std::to_string(t.bn), bks = std::to_string(t.bks);
    if (!f.n) return refuse(f.err + (": N % " + bn + " and K % " + bks + " must be 0"));
    if (a.N % t.bn) return refuse(f.n + (": N must be a multiple of the tile width " + bn));
    return refuse(f.k + (": K must be a multiple of the stage depth " + bks));
  }
  enqueue(t.kern, dim3(pinned_grid(units, unsigned(a.ctl >> 20) & 0xffu)), dim3(t.threads), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_err = std::string(f.err) + ": " + hipGetErrorString(e);
    return int(e);
  }
  return 0;
}

// the operands as the entry points take them
X3Args x3_args(const void* A, size_t ap, const void* W, size_t wp, const float* bias, const float* R, const float* R2,
               int r2_rows, float* C, void* Cp, size_t cp, int M, int N, int K, int ctl, void* stream) {
  return {A, ap, reinterpret_cast<const __bf16*>(W), wp, bias, R, R2, r2_rows, C, reinterpret_cast<__bf16*>(Cp), cp,
          M, N, K, ctl, 0, reinterpret_cast<hipStream_t>(stream)};
}

bool epi_operands_missing(const X3Args& a) {
  return ((a.ctl & EPI_BIAS) && !a.bias) || ((a.ctl & EPI_RES) && !a.R) ||
         ((a.ctl & EPI_RES2) && (!a.R2 || a.r2_rows <= 0));
}

int dispatch(const X3Args& a, int cfg) {
  const Config<KernP>* t = pick(kTiles, cfg);
  return t ? launch(*t, tile_units(*t, a), a) : refuse("gemm_x3: unknown tile config");
}
}  // namespace

static int g_group_m = 1;
static int g_ablate = 0;  // timing studies only: 1 = skip the A operand loads, 2 = skip W (results invalid)

// The control word of a launch above its epilogue flags: tile rows per group (bits 8-15), ablation
// (16-18), the XCD pin mask (20-27); nos_gemm_x3_partials adds splits - 1 (28-30).
static int x3_ctl(int epi) { return epi | (g_group_m << 8) | (g_ablate << 16) | int(nos_pin_mask() << 20); }

extern "C" {

const char* nos_gemm_x3_last_error() { return g_err.c_str(); }

int nos_gemm_x3_set_ablate(int a) {
  g_ablate = a & 7;
  return 0;
}

// grouped tile order (tile rows per group, 1..255; 1 = row-major): see tile_rc
int nos_gemm_x3_set_group(int g) {
  if (g < 1 || g > 255) return refuse("gemm_x3: group must be 1..255");
  g_group_m = g;
  return 0;
}

// The tile schedule of a launch over tiles_m x tiles_n tiles, walked on the host with the kernels'
// own functions (x3_schedule.h, pin.h). persistent != 0: gemm_x3s asked for `grid` workgroups
// (clamped as its launch clamps it); otherwise one unit = (tile, split) per workgroup and `grid` is
// not used. hdr = {P logical workgroups, nx XCDs they are dealt over, units the launch must cover,
// physical grid, units the schedule runs}; wg[3w..] = {count, base, stride} of logical workgroup w
// (w < P <= wg_cap); units[4i..] = {logical tile, mt, nt, split} in workgroup order, each
// workgroup's in stream order (the first unit_cap of them).
int nos_gemm_x3_schedule(int tiles_m, int tiles_n, int group, int grid, unsigned pin, int persistent, int splits,
                         int* hdr, int* wg, int wg_cap, int* units, int unit_cap) {
  if (tiles_m < 1 || tiles_n < 1 || tiles_m > (1 << 20) / tiles_n || group < 1 || group > 255 || pin > 0xffu ||
      splits < 1 || splits > 8 || (persistent && splits != 1) || !hdr || !wg || !units) {
    g_err = "gemm_x3 schedule: tiles >= 1 (at most 2^20), group 1..255, an 8-bit pin, splits 1..8 (1 if persistent)";
    return -1;
  }
  const int tiles = tiles_m * tiles_n, want = tiles * splits;
  const unsigned phys = pinned_grid(unsigned(persistent ? x3s_grid(grid, tiles) : want), pin);
  const int nx = pin ? __builtin_popcount(pin) : 8, P = pin ? pinned_n(phys, nx) : int(phys);
  if (P > wg_cap) {
    g_err = "gemm_x3 schedule: " + std::to_string(P) + " workgroups do not fit wg_cap";
    return -1;
  }
  int n = 0;
  auto put = [&](int t, int mt, int nt, int sp) {
    if (n < unit_cap) units[4 * n] = t, units[4 * n + 1] = mt, units[4 * n + 2] = nt, units[4 * n + 3] = sp;
    ++n;
  };
  for (int w = 0; w < P; ++w) {
    int base = 0, stride = 0, count = 0, mt = 0, nt = 0, sp = 0;
    if (persistent) {
      xcd_band(w, P, nx, tiles, base, stride, count);
      for (int i = 0; i < count; ++i) {
        tile_rc(base + i * stride, tiles_m, tiles_n, group, mt, nt);
        put(base + i * stride, mt, nt, 0);
      }
    } else if (int t = 0; x3_unit(w, P, nx, tiles, splits, t, sp)) {
      tile_rc(t, tiles_m, tiles_n, group, mt, nt);
      base = xcd_major_n(w, P, nx), count = 1;
      put(t, mt, nt, sp);
    }
    wg[3 * w] = count, wg[3 * w + 1] = base, wg[3 * w + 2] = stride;
  }
  hdr[0] = P, hdr[1] = nx, hdr[2] = want, hdr[3] = int(phys), hdr[4] = n;
  return 0;
}

int nos_gemm_x3_num_configs() { return table_size(kTiles); }

// (BM, BN, LDS buffers) of tile id cfg: a config of nos_gemm_x3, or 100 + a config of nos_gemm_x3_persistent
int nos_gemm_x3_tile(int cfg, int* bm, int* bn, int* nbuf) {
  const Config<KernP>* t = cfg >= kPersistentBase ? pick(kPersistent, cfg - kPersistentBase) : pick(kTiles, cfg);
  if (!t) return -1;
  *bm = t->bm, *bn = t->bn, *nbuf = t->nbuf;
  return 0;
}

// C[M,N] = A[M,K] · W[N,K]^T with A and W as three bf16 planes (plane strides ap, wp elements,
// 16-B aligned), fused epilogue flags as nos_gemm_f32 (1 bias, 2 GELU, 4 + R, 8 + R2[row % r2_rows]).
// Output: fp32 C (may be null) and/or three bf16 planes Cp (plane stride cp; may be null).
// K % 32 == 0, N % BN == 0, row-major contiguous operands.
int nos_gemm_x3(const void* A, size_t ap, const void* W, size_t wp, const float* bias, const float* R,
                const float* R2, int r2_rows, float* C, void* Cp, size_t cp, int M, int N, int K, int epi, int cfg,
                void* stream) {
  const X3Args a = x3_args(A, ap, W, wp, bias, R, R2, r2_rows, C, Cp, cp, M, N, K, x3_ctl(epi), stream);
  if (K % BK || ap % 8 || wp % 8 || cp % 8)
    return refuse("gemm_x3: K must be a multiple of 32 and plane strides multiples of 8 elements");
  if (!C && !Cp) return refuse("gemm_x3: no output");
  if (epi_operands_missing(a)) return refuse("gemm_x3: epilogue operand missing");
  return dispatch(a, cfg);
}

// Persistent stream-of-stages GEMM (same operands/epilogue as nos_gemm_x3) with an explicit grid
// (workgroups; the caller sizes it to the slice: CUs x resident workgroups per CU); cfg: kPersistent.
int nos_gemm_x3_persistent(const void* A, size_t ap, const void* W, size_t wp, const float* bias, const float* R,
                           const float* R2, int r2_rows, float* C, void* Cp, size_t cp, int M, int N, int K, int epi,
                           int cfg, int grid, void* stream) {
  const X3Args a = x3_args(A, ap, W, wp, bias, R, R2, r2_rows, C, Cp, cp, M, N, K, x3_ctl(epi), stream);
  if (K % BK || ap % 8 || wp % 8 || cp % 8 || (!C && !Cp))
    return refuse("gemm_x3s: K % 32 (K % 64 for 64-deep stages), plane strides % 8, and an output are required");
  if (epi_operands_missing(a)) return refuse("gemm_x3s: epilogue operand missing");
  const Config<KernP>* t = pick(kPersistent, cfg);
  return t ? launch(*t, x3s_grid(grid, tile_units(*t, a)), a) : refuse("gemm_x3s: unknown config");
}

// Split-K partial sums of C = A · W^T (the LDS-DMA tiles): plane s of C [splits][M][N] fp32
// holds the K stages [s*nk/splits, (s+1)*nk/splits); no epilogue (the consumer adds the planes in
// order, then bias and residuals: splitk_layernorm in kernels.hip). 2 <= splits <= min(8, K/stage).
int nos_gemm_x3_partials(const void* A, size_t ap, const void* W, size_t wp, float* C, int M, int N, int K, int cfg,
                         int splits, void* stream) {
  if (K % BK || ap % 8 || wp % 8 || !C) return refuse("gemm_x3 partials: K % 32, plane strides % 8 and an output");
  if (cfg < kFirstDma || cfg >= table_size(kTiles) || splits < 2 || splits > 8 || splits > K / BK)
    return refuse("gemm_x3 partials: an LDS-DMA config (" + std::to_string(kFirstDma) + ".." +
                  std::to_string(table_size(kTiles) - 1) + ") and 2..8 splits");
  return dispatch(x3_args(A, ap, W, wp, nullptr, nullptr, nullptr, 0, C, nullptr, 0, M, N, K,
                          x3_ctl(0) | ((splits - 1) << 28), stream),
                  cfg);
}

// The work split a stream-K launch of `P` workgroups uses (P clamped to the unit count):
// out = {P, U, nk, bm, bn, tiles_n, planes}; planes = the most segments any tile has, the depth
// of the fp32 partial buffer [planes][M][N] the launch writes. cfg: kStreamK.
int nos_gemm_x3_streamk_map(int M, int N, int K, int cfg, int P, int* out) {
  const Config<KernK>* c = pick(kStreamK, cfg);
  if (!c || M <= 0 || P <= 0)
    return refuse("gemm_x3k: config 0.." + std::to_string(table_size(kStreamK) - 1) + ", M > 0 and P > 0");
  const int bm = c->bm, bn = c->bn, bks = c->bks;
  if (N % bn || K % bks) {
    g_err = "gemm_x3k: N % " + std::to_string(bn) + " and K % " + std::to_string(bks) + " must be 0";
    return -1;
  }
  SkMap m{0, 0, K / bks, bm, bn, N / bn};
  const long long tiles = (long long)((M + bm - 1) / bm) * m.tiles_n;
  if (tiles * m.nk > (1LL << 30) / 4096) return refuse("gemm_x3k: too many units");
  m.U = int(tiles * m.nk);
  m.P = std::min(P, m.U);
  int planes = 1;
  for (int t = 0; t < int(tiles); ++t) planes = std::max(planes, sk_segments(t, m));
  const int v[7] = {m.P, m.U, m.nk, bm, bn, m.tiles_n, planes};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
  return 0;
}

// Raw partial sums of C = A · W^T, stream-K over P workgroups (P from nos_gemm_x3_streamk_map):
// C is the [planes][M][N] fp32 buffer; no epilogue (splitk_layernorm with the same map adds them).
int nos_gemm_x3_streamk(const void* A, size_t ap, const void* W, size_t wp, float* C, int M, int N, int K, int cfg,
                        int P, void* stream) {
  int m[7];
  if (nos_gemm_x3_streamk_map(M, N, K, cfg, P, m) != 0) return -1;
  if (m[0] != P || ap % 8 || wp % 8 || !C)
    return refuse("gemm_x3k: P must be the map's (clamped) P; plane strides % 8; an output");
  // gemm_x3k reads the ablation and pin bits of the control word only (the group bits ride along unread)
  X3Args a = x3_args(A, ap, W, wp, nullptr, nullptr, nullptr, 0, C, nullptr, 0, M, N, K, x3_ctl(0), stream);
  a.P = P;
  return launch(kStreamK[cfg], P, a);
}

// C = A · W^T with A as fp32 rows [M][K] (split into planes in the kernel) and W as three bf16
// planes; epilogue and outputs as nos_gemm_x3. cfg: kF32A.
int nos_gemm_x3_f32a(const float* A, const void* W, size_t wp, const float* bias, const float* R, const float* R2,
                     int r2_rows, float* C, void* Cp, size_t cp, int M, int N, int K, int epi, int cfg,
                     void* stream) {
  const X3Args a = x3_args(A, 0, W, wp, bias, R, R2, r2_rows, C, Cp, cp, M, N, K, x3_ctl(epi), stream);
  if (!A || K % 32 || wp % 8 || cp % 8 || (!C && !Cp))
    return refuse("gemm_x3a: an fp32 A, K % 32, plane strides % 8 and an output are required");
  if (epi_operands_missing(a)) return refuse("gemm_x3a: epilogue operand missing");
  const Config<KernA>* t = pick(kF32A, cfg);
  return t ? launch(*t, tile_units(*t, a), a) : refuse("gemm_x3a: unknown config");
}

}  // extern "C"
