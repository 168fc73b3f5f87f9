// LDS-DMA pieces of the x3 GEMMs (gemm_x3.hip): the operand tiles go global -> LDS with
// global_load_lds_dwordx4 (no register staging), S LDS buffers deep, so S-1 stages of loads are in
// flight behind the MFMAs at the cost of LDS only. The DMA writes a wave's 64 lanes x 16 B
// lane-linearly, so the image has unpadded 64-B rows [plane][row][4 chunks] and conflict-freedom
// comes from the lane -> chunk map instead: LDS slot c of row r holds k-chunk c ^ ((r >> 2) & 3); a
// fragment read of chunk 2s+h then lands, over any ds_read_b128 lane group, on 16 distinct 16-B bank
// slots (r mod 4 picks the 16-bank quarter, (r >> 2) & 3 the slot inside it). One raw s_barrier per
// stage: a __syncthreads() fence would wait for every outstanding DMA (vmcnt(0)) and serialise the
// pipeline; the per-wave "stage ks landed" wait is an explicit vmcnt(loads of the S-2 younger
// stages). Here: the waits, the swizzle, one stage's DMA, the geometry of a workgroup's waves over
// its tile, and the S-stage ring itself (X3_RING), written once for gemm_x3d / gemm_x3s / gemm_x3k.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

typedef __attribute__((address_space(3))) void lds_void;

template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}

// Wait until this wave's DMA of the current stage has landed when `rem` younger stages (at most
// S-2) have been issued behind it: vmcnt needs an immediate, so the tail of the K loop (fewer
// younger stages in flight) takes the smaller waits by a wave-uniform branch.
template <int S, int NLD>
__device__ __forceinline__ void vm_wait_stage(int rem) {
  const int r = min(S - 2, rem);
  if constexpr (S > 3) {
    if (r >= 2) {
      vm_wait<2 * NLD>();
      return;
    }
  }
  if constexpr (S > 2) {
    if (r >= 1) {
      vm_wait<NLD>();
      return;
    }
  }
  vm_wait<0>();
}

__device__ __forceinline__ void raw_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Stage depth BKS (32 or 64 bf16 per plane) sets the LDS row: CPR = BKS/8 16-byte chunks, so one
// wave DMA instruction (64 lanes x 16 B) covers RPI = 64/CPR rows. BKS = 64 reads whole 128-byte
// row segments: half the cache lines per byte moved of BKS = 32 (the texture-address path, not
// HBM, bounds these short-K GEMMs even when every line hits L2). Chunk c of local row r sits at
// slot c ^ swz(r), swz(r) = (r / (16/CPR)) % CPR, which makes the fragment reads (lanes j, j+32
// on rows j of a 32-row block) conflict-free for both depths.
template <int BKS, bool M16 = false>
__device__ __forceinline__ int dma_swz(int r) {
  if constexpr (M16) {
    // 16x16x32 fragment reads (lane l: row l%16, chunk l/16 of a 64-byte row): slot c ^ 2((r>>2)&1)
    // puts every ds_read_b128 lane group on 16 distinct 16-byte bank slots
    static_assert(BKS == 32, "the 16x16x32 image is defined for 32-deep stages");
    return ((r >> 2) & 1) << 1;
  } else {
    constexpr int CPR = BKS / 8;
    return (r / (16 / CPR)) % CPR;
  }
}

// Per-lane byte offsets of this wave's DMA rows inside one plane (fixed for the whole K loop):
// row groups g = wave + NW*i of RPI rows; lane -> row RPI*g + lane/CPR, chunk (lane%CPR) ^ swz(row).
template <int ROWS, int NW, int BKS = 32, bool M16 = false>
__device__ __forceinline__ void dma_offsets(uint32_t (&voff)[ROWS * BKS / 512 / NW], int r0, int rmax, int K,
                                            int wave, int lane) {
  constexpr int CPR = BKS / 8, RPI = 64 / CPR;
#pragma unroll
  for (int i = 0; i < ROWS / RPI / NW; ++i) {
    const int rl = RPI * (wave + NW * i) + lane / CPR;
    const int c = (lane % CPR) ^ dma_swz<BKS, M16>(rl);
    const int row = min(r0 + rl, rmax);
    voff[i] = uint32_t(row) * uint32_t(K) * 2u + 16u * uint32_t(c);
  }
}

// one stage of ROWS x BKS bf16 per plane for this wave (NW waves share the row groups): a
// wave-uniform base (plane, k0) plus the lane's fixed 32-bit offset, so the loads take the
// SGPR-base + VGPR-offset form and a stage costs no per-lane address arithmetic
template <int ROWS, int NW, int BKS = 32>
__device__ __forceinline__ void dma_stage(const __bf16* __restrict__ X, size_t plane,
                                          const uint32_t (&voff)[ROWS * BKS / 512 / NW], int k0, __bf16* lds,
                                          int wave) {
  constexpr int RPI = 512 / BKS;
#pragma unroll
  for (int i = 0; i < ROWS / RPI / NW; ++i) {
    const int g = wave + NW * i;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const char* src = reinterpret_cast<const char*>(X + q * plane + k0) + voff[i];
      __builtin_amdgcn_global_load_lds(src, (lds_void*)(lds + q * ROWS * BKS + RPI * g * BKS), 16, 0, 0);
    }
  }
}

// A BM x BN tile on a WGM x WGN grid of waves, BKS-deep stages: the constants every LDS-DMA kernel
// derives from its template parameters.
template <int BM, int BN, int WGM, int WGN, int BKS = 32>
struct X3Waves {
  static constexpr int NW = WGM * WGN;
  static constexpr int WM = BM / WGM, WN = BN / WGN;
  static constexpr int TM = WM / 32, TN = WN / 32;      // 32x32 accumulators per wave
  static constexpr int TM16 = WM / 16, TN16 = WN / 16;  // 16x16 accumulators per wave
  static constexpr int RPI = 512 / BKS;                 // rows per DMA instruction
  static constexpr int VA = BM / RPI / NW, VB = BN / RPI / NW;  // row groups of A, B per wave
  static_assert(BM % (RPI * NW) == 0 && BN % (RPI * NW) == 0, "row groups must divide over the waves");
  static constexpr int NLD = 3 * VA + 3 * VB;  // DMA instructions per wave per stage
};

}  // namespace

// ---- pieces that expand in the kernel's own scope ----------------------------------------------
// They are macros, not functions or lambdas, because the kernels' instruction streams depend on it:
// a lambda's captures reach the interprocedural passes, which run before inlining, as loads from a
// closure, and value ranges the kernels' address arithmetic relies on (the 8-bit group of tile_rc
// for one) were then lost in every kernel of the file, the ones that use none of this included; a
// helper function around two dma_stage calls changed the register allocation of its callers.

// this thread's place in the workgroup as locals of the kernel: lane, wave, the wave's place
// (wm, wn) on the WGM x WGN grid, and the lane's column j and half hf of a 32x32 accumulator
#define X3_WAVE_LOCALS(WGN)                                                                            \
  const int tid = threadIdx.x, lane = tid & 63;                                                        \
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6); /* wave-uniform: LDS bases stay scalar */ \
  const int wm = wave / (WGN), wn = wave % (WGN);                                                      \
  [[maybe_unused]] const int j = lane & 31, hf = lane >> 5

// ACC[R][C] = 0, for accumulators of vector type V
#define X3_ZERO_ACC(ACC, R, C, V)                 \
  _Pragma("unroll") for (int a = 0; a < (R); ++a) \
      _Pragma("unroll") for (int b = 0; b < (C); ++b) ACC[a][b] = V{0};

// Both operands' stage at K0 into the stage buffers (AS, BS), with the kernel's own names for the
// operands (A, a_plane, W, w_plane), its tile constants (BM, BN, NW, BKS), wave and ablate (timing
// studies skip A (1) or W (2)); VA, VB are the lane offsets of dma_offsets.
#define X3_DMA_AB(VA, VB, K0, AS, BS)                                        \
  {                                                                          \
    if (!(ablate & 1)) dma_stage<BM, NW, BKS>(A, a_plane, VA, K0, AS, wave); \
    if (!(ablate & 2)) dma_stage<BN, NW, BKS>(W, w_plane, VB, K0, BS, wave); \
  }
// the same for a stream that changes tile from stage to stage (gemm_x3s, gemm_x3k): the stage of the
// tile at rows M0 of A and N0 of W, its lane offsets worked out here (M, N, K, lane: the kernel's)
#define X3_DMA_AB_AT(M0, N0, K0, AS, BS)                         \
  {                                                              \
    uint32_t va_[BM * BKS / 512 / NW], vb_[BN * BKS / 512 / NW]; \
    dma_offsets<BM, NW, BKS>(va_, M0, M - 1, K, wave, lane);     \
    dma_offsets<BN, NW, BKS>(vb_, N0, N - 1, K, wave, lane);     \
    X3_DMA_AB(va_, vb_, K0, AS, BS)                              \
  }

// The stage buffers A0..A3, B0..B3 of a kernel, S of them in use. One __shared__ object per stage
// buffer: the compiler's LDS-DMA wait tracking can then tell the buffer being read from the
// buffers being filled (one array indexed by stage would make every fragment read wait for ALL
// outstanding DMA, vmcnt(0), and serialise the pipeline).
#define X3_STAGE_BUFFERS(S, BM, BN, BKS)                                                     \
  __shared__ __attribute__((aligned(16))) __bf16 A0[3 * (BM) * (BKS)], A1[3 * (BM) * (BKS)], \
      A2[(S) > 2 ? 3 * (BM) * (BKS) : 8], A3[(S) > 3 ? 3 * (BM) * (BKS) : 8];                \
  __shared__ __attribute__((aligned(16))) __bf16 B0[3 * (BN) * (BKS)], B1[3 * (BN) * (BKS)], \
      B2[(S) > 2 ? 3 * (BN) * (BKS) : 8], B3[(S) > 3 ? 3 * (BN) * (BKS) : 8]
// stage buffer b of those a kernel declared (b past its last buffer is never asked for)
#define X3_BUF(b, P0, P1, P2, P3) ((b) == 0 ? P0 : (b) == 1 ? P1 : (b) == 2 ? P2 : P3)
#define X3_A(b) X3_BUF(b, A0, A1, A2, A3)
#define X3_B(b) X3_BUF(b, B0, B1, B2, B3)

// The S-stage ring over a stream of TOTAL stages, expanded in the kernel's own scope. The kernel
// gives two statement macros: ISSUE(h, b) starts the DMA of stream position h into stage buffer
// b = h % S; CONSUME(g, b) runs position g's MFMAs from buffer b (and whatever ends a tile or a
// segment there). S-1 stages are in flight behind the stage being consumed. No DMA is issued past
// the last stage, so when the ring ends no load can still be landing in a stage buffer (and no
// bandwidth goes to dead re-reads). The steady loop only runs while every issue is in range (static
// vmcnt, unconditional DMA); the last iterations run a tail with a bounds-checked issue and the
// smaller waits (vm_wait_stage). NLD = DMA instructions per wave per stage.
#define X3_RING_STEP(S, NLD, G, BUF, ISSUE, CONSUME)                                  \
  {                                                                                   \
    vm_wait<((S) - 2) * (NLD)>(); /* this wave's DMA of position G has landed */      \
    raw_barrier();                /* everyone's has; position G-1's buffer is free */ \
    ISSUE((G) + (S) - 1, ((BUF) + (S) - 1) % (S))                                     \
    __builtin_amdgcn_sched_barrier(0); /* issue the DMA before the stage's MFMAs */   \
    CONSUME(G, BUF)                                                                   \
  }
#define X3_RING(S, NLD, TOTAL, ISSUE, CONSUME)                                       \
  {                                                                                  \
    static_assert((S) >= 2 && (S) <= 4, "2-4 LDS stages");                           \
    const int total_ = (TOTAL);                                                      \
    for (int st_ = 0; st_ < (S) - 1; ++st_)                                          \
      if (st_ < total_) ISSUE(st_, st_)                                              \
    int g_ = 0;                                                                      \
    for (; g_ + 2 * (S) - 1 <= total_; g_ += (S)) {                                  \
      X3_RING_STEP(S, NLD, g_, 0, ISSUE, CONSUME)                                    \
      X3_RING_STEP(S, NLD, g_ + 1, 1, ISSUE, CONSUME)                                \
      if constexpr ((S) > 2) X3_RING_STEP(S, NLD, g_ + 2, 2, ISSUE, CONSUME)         \
      if constexpr ((S) > 3) X3_RING_STEP(S, NLD, g_ + 3, 3, ISSUE, CONSUME)         \
    }                                                                                \
    for (; g_ < total_; ++g_) {                                                      \
      const int buf_ = g_ % (S);                                                     \
      vm_wait_stage<(S), (NLD)>(total_ - 1 - g_);                                    \
      raw_barrier();                                                                 \
      if (g_ + (S) - 1 < total_) ISSUE(g_ + (S) - 1, (buf_ + (S) - 1) % (S))         \
      __builtin_amdgcn_sched_barrier(0);                                             \
      CONSUME(g_, buf_)                                                              \
    }                                                                                \
    vm_wait<0>(); /* no DMA may still target this workgroup's LDS when it retires */ \
  }
