// nos workload kernels for gfx950 (MI355X): flash attention on the f32-input matrix cores.
//
//  * attn_fwd_f32 / attn_fwd_sk / attn_fwd_sk_lds (the f32-MFMA path, set_fp32_matmul("f32")): flash attention over a packed [B, T, 3*H*64] fp32 QKV tensor on the exact-fp32
//    matrix cores (v_mfma_f32_32x32x2_f32, 64 FLOP/clk/SIMD). One wave owns 32 queries of one head.
//    It computes S^T = K Q^T so that every lane owns ONE query column: the softmax row reductions
//    are 16 in-register ops plus a single cross-half exchange (lane l <-> l^32), no LDS. The
//    accumulator of S^T is fed straight back as the B operand of O^T += V^T P^T (accumulator-as-
//    operand, cdna_hip_programming.md §3), so P never leaves registers. Head-dim -> MFMA K-slot
//    assignment is dim = 32*half + step, which makes every lane's Q and K fragment one contiguous
//    128-byte run (8 x dwordx4). K/V of one head (3401 x 64 x 4 B x 2 = 1.7 MB) stays L2-resident
//    across the query tiles of that head. The production launch is stream-K (attn_fwd_sk): a
//    persistent grid sized to the slice's resident-wave capacity splits the (query tile x key
//    block) work evenly, so a 32-CU CPX slice and the whole 256-CU GPU are both tail-free.
#include <hip/hip_runtime.h>

#include "err.h"
#include "x3_common.h"

#include <cmath>
#include <cstdint>

namespace {

// ------------------------------------------------------------------------------------------
// Flash attention, fp32, head_dim 64.
// (HD, key_of, half_max, half_sum: x3_common.h)

// Online-softmax flash attention over key blocks [kb0, kb1) (32 keys each) for the 32 queries
// q0..q0+31 of one head. Returns the unnormalised O^T accumulators and the running (m, l).
struct AttnAcc {
  f32x16 o0, o1;
  float m, l;
};

__device__ __forceinline__ AttnAcc attn_segment(const float* __restrict__ base, int q0, int head, int kb0, int kb1,
                                                int T, int D, float scale_log2e) {
  const int lane = threadIdx.x & 63;
  const int j = lane & 31, hf = lane >> 5;
  const int ld = 3 * D;
  // Q^T fragment: Q[q0 + j][32*hf + s], s = 0..31, pre-scaled into the log2 domain
  float qreg[32];
  {
    const int qrow = min(q0 + j, T - 1);
    const float4* qp = reinterpret_cast<const float4*>(base + size_t(qrow) * ld + head * HD + 32 * hf);
#pragma unroll
    for (int s4 = 0; s4 < 8; ++s4) {
      const float4 v = qp[s4];
      qreg[4 * s4 + 0] = v.x * scale_log2e;
      qreg[4 * s4 + 1] = v.y * scale_log2e;
      qreg[4 * s4 + 2] = v.z * scale_log2e;
      qreg[4 * s4 + 3] = v.w * scale_log2e;
    }
  }
  AttnAcc a;
  a.o0 = f32x16{0};
  a.o1 = f32x16{0};
  a.m = -INFINITY;
  a.l = 0.f;
  const float* kbase = base + D + head * HD + 32 * hf;
  const float* vbase = base + 2 * D + head * HD + j;

  for (int blk = kb0; blk < kb1; ++blk) {
    const int kb = blk * 32;
    // K fragment: K[kb + j][32*hf + s]
    float kreg[32];
    {
      const int krow = min(kb + j, T - 1);
      const float4* kp = reinterpret_cast<const float4*>(kbase + size_t(krow) * ld);
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4) {
        const float4 v = kp[s4];
        kreg[4 * s4 + 0] = v.x;
        kreg[4 * s4 + 1] = v.y;
        kreg[4 * s4 + 2] = v.z;
        kreg[4 * s4 + 3] = v.w;
      }
    }
    // V operands for this block, issued early to overlap the S^T MFMAs: V[kb + key(t, hf)][j], [32 + j]
    float v0[16], v1[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int vrow = min(kb + key_of(t, hf), T - 1);
      v0[t] = vbase[size_t(vrow) * ld];
      v1[t] = vbase[size_t(vrow) * ld + 32];
    }
    // S^T[key][query] = sum_d K[key][d] Q[query][d]
    f32x16 s = {0};
#pragma unroll
    for (int st = 0; st < 32; ++st) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kreg[st], qreg[st], s, 0, 0, 0);

    if (kb + 32 > T) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kb + key_of(r, hf) >= T) s[r] = -INFINITY;
    }
    float mx = s[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
    mx = half_max(mx);
    const float m_new = fmaxf(a.m, mx);
    const float alpha = __builtin_amdgcn_exp2f(a.m - m_new);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = __builtin_amdgcn_exp2f(s[r] - m_new);
      psum += s[r];
    }
    psum = half_sum(psum);
    a.l = a.l * alpha + psum;
    a.m = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      a.o0[r] *= alpha;
      a.o1[r] *= alpha;
    }
    // O^T[d][query] += sum_key V^T[d][key] P^T[key][query]; P^T register t is key key_of(t, hf)
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      a.o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[t], s[t], a.o0, 0, 0, 0);
      a.o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[t], s[t], a.o1, 0, 0, 0);
    }
  }
  return a;
}

__device__ __forceinline__ void attn_store_out(const AttnAcc& a, float* __restrict__ out, int b, int q0, int head,
                                               int T, int D) {
  const int lane = threadIdx.x & 63;
  const int j = lane & 31, hf = lane >> 5;
  const int q = q0 + j;
  if (q >= T) return;
  const float inv = 1.f / a.l;
  float* orow = out + (size_t(b) * T + q) * D + head * HD;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int d = key_of(r, hf);
    orow[d] = a.o0[r] * inv;
    orow[32 + d] = a.o1[r] * inv;
  }
}

// One wave per (query tile, head, batch): the whole key range, normalised output. Used when no
// workspace is available (nos_attention_f32).
__global__ __launch_bounds__(64, 2) void attn_fwd_f32(const float* __restrict__ qkv, float* __restrict__ out, int T,
                                                      int H, float scale_log2e) {
  const int qt = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int D = H * HD;
  const AttnAcc a = attn_segment(qkv + size_t(b) * T * 3 * D, qt * 32, head, 0, (T + 31) / 32, T, D, scale_log2e);
  attn_store_out(a, out, b, qt * 32, head, T, D);
}

// ---- stream-K attention ----------------------------------------------------------------------
// The work is U = B*H*QT*NK units (one 32-query x 32-key block each, QT = NK = ceil(T/32)), laid out
// tile-major so consecutive units share a head's K/V. A persistent grid of exactly P waves (slice
// CUs x resident waves per CU) gives wave w the contiguous range [w*U/P, (w+1)*U/P): every SIMD of
// the slice gets the same number of MFMAs, so there is no wave-quantisation tail whatever the slice
// size (a fixed split count leaves 1.25 or 2.5 "rounds" for 256 or 32 CUs). Segments covering a
// whole tile are normalised and stored directly; a wave's first and last segments may be partial
// and go to its two workspace slots, merged by attn_sk_fixup (a second launch on the same stream,
// so no inter-wave spin-waits exist). Logical wave ids are XCD-major: hardware round-robins
// workgroups over the 8 XCDs, so remapping keeps each XCD on a contiguous run of units and its
// 4 MB L2 holds at most two heads' K/V (1.7 MB each at T=3401) instead of all of them.
// (sk_begin, sk_logical: x3_common.h)

template <int WPE>
__global__ __launch_bounds__(64, WPE) void attn_fwd_sk(const float* __restrict__ qkv, float* __restrict__ out,
                                                     float* __restrict__ part_o, float* __restrict__ part_ml, int B,
                                                     int T, int H, float scale_log2e, int P) {
  const int w = sk_logical(blockIdx.x, P);
  const int NK = (T + 31) / 32, QT = NK;
  const long long U = (long long)B * H * QT * NK;
  long long u = sk_begin(w, U, P);
  const long long u1 = sk_begin(w + 1, U, P);
  const int D = H * HD;
  const int lane = threadIdx.x & 63;
  const int j = lane & 31, hf = lane >> 5;
  bool first = true;
  while (u < u1) {
    const long long tile = u / NK;
    const int kb0 = int(u - tile * NK);
    const int kb1 = int(min<long long>(NK, kb0 + (u1 - u)));
    const int qt = int(tile % QT);
    const int head = int((tile / QT) % H);
    const int b = int(tile / ((long long)QT * H));
    const AttnAcc a = attn_segment(qkv + size_t(b) * T * 3 * D, qt * 32, head, kb0, kb1, T, D, scale_log2e);
    if (kb0 == 0 && kb1 == NK) {
      attn_store_out(a, out, b, qt * 32, head, T, D);
    } else {
      // slot layout: part_o[slot][d][32 queries] (lane-contiguous stores), part_ml[slot][2][32]
      const size_t slot = size_t(w) * 2 + (first ? 0 : 1);
      float* po = part_o + slot * (HD * 32);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int d = key_of(r, hf);
        po[d * 32 + j] = a.o0[r];
        po[(32 + d) * 32 + j] = a.o1[r];
      }
      if (hf == 0) {
        part_ml[slot * 64 + j] = a.m;
        part_ml[slot * 64 + 32 + j] = a.l;
      }
    }
    u += kb1 - kb0;
    first = false;
  }
}

// Merge the partial segments of every tile that more than one wave touched. One 256-thread block
// per tile: thread = (query quad, d); contributors are the waves whose ranges intersect the tile.
__global__ __launch_bounds__(256) void attn_sk_fixup(const float* __restrict__ part_o,
                                                     const float* __restrict__ part_ml, float* __restrict__ out,
                                                     int B, int T, int H, int P) {
  const int NK = (T + 31) / 32, QT = NK;
  const long long U = (long long)B * H * QT * NK;
  const long long tile = blockIdx.x;
  const long long t0 = tile * NK, t1 = t0 + NK;  // unit range of this tile
  // wave containing unit u: largest w with w*U/P <= u
  const long long w_lo = ((t0 + 1) * P + U - 1) / U - 1;
  const long long w_hi = (t1 * P + U - 1) / U - 1;
  if (w_lo == w_hi) return;  // one wave did the whole tile and stored it normalised
  const int qt = int(tile % QT);
  const int head = int((tile / QT) % H);
  const int b = int(tile / ((long long)QT * H));
  const int D = H * HD;
  const int d = threadIdx.x & 63;
  for (int jq = threadIdx.x >> 6; jq < 32; jq += 4) {
    const int q = qt * 32 + jq;
    if (q >= T) break;
    float mmax = -INFINITY;
    for (long long w = w_lo; w <= w_hi; ++w) {
      const long long s = w * U / P;
      if (s == (w + 1) * U / P) continue;
      const size_t slot = size_t(w) * 2 + (s >= t0 ? 0 : 1);
      mmax = fmaxf(mmax, part_ml[slot * 64 + jq]);
    }
    float num = 0.f, den = 0.f;
    for (long long w = w_lo; w <= w_hi; ++w) {
      const long long s = w * U / P;
      if (s == (w + 1) * U / P) continue;
      const size_t slot = size_t(w) * 2 + (s >= t0 ? 0 : 1);
      const float sc = __builtin_amdgcn_exp2f(part_ml[slot * 64 + jq] - mmax);
      num += part_o[slot * (HD * 32) + d * 32 + jq] * sc;
      den += part_ml[slot * 64 + 32 + jq] * sc;
    }
    out[(size_t(b) * T + q) * D + head * HD + d] = num / den;
  }
}


// ---- stream-K attention, LDS-shared K/V (production path) --------------------------------------
// A 256-thread workgroup = 4 waves = 4 consecutive 32-query tiles (a 128-query "group") of one
// head. The workgroup streams 32-key blocks of K and V through LDS once for all four waves
// (coalesced dwordx4 global loads, register-prefetched one block ahead, double-buffered, one
// barrier per block), so L2->CU traffic and texture-address work drop 4x versus every wave
// fetching its own fragments (the v1 kernel above is TA-bound at ~640 cache-line lookups per wave
// per block). LDS images: K row-major with a 68-float stride — the per-lane ds_read_b128 of
// K[key=j][32*hf + 4*s4] then hits 16 distinct 16-B slots per lane group (17*j mod 16); V
// row-major (stride 64), read as ds_read_b32 V[key][j] with 32 consecutive banks per half-wave.
// Stream-K runs over (group x key block) units with a persistent grid of P workgroups, the same
// first/last-segment workspace scheme and XCD-major order as attn_fwd_sk.
constexpr int KSTR = 68, VSTR = 64;
constexpr int KBUF = 32 * KSTR, VBUF = 32 * VSTR;

__global__ __launch_bounds__(256, 2) void attn_fwd_sk_lds(const float* __restrict__ qkv, float* __restrict__ out,
                                                          float* __restrict__ part_o, float* __restrict__ part_ml,
                                                          int B, int T, int H, float scale_log2e, int P) {
  __shared__ __attribute__((aligned(16))) float lds_k[2 * KBUF];
  __shared__ __attribute__((aligned(16))) float lds_v[2 * VBUF];
  const int w = sk_logical(blockIdx.x, P);
  const int NK = (T + 31) / 32, QT = NK, QG = (QT + 3) / 4;
  const long long U = (long long)B * H * QG * NK;
  long long u = sk_begin(w, U, P);
  const long long u1 = sk_begin(w + 1, U, P);
  const int D = H * HD, ld = 3 * D;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int j = lane & 31, hf = lane >> 5;
  // cooperative-load mapping: float4 f = tid + 256*i, i = 0..1 -> key row f/16, dims 4*(f%16)
  const int lrow = tid >> 4, lc4 = tid & 15;
  bool first = true;
  while (u < u1) {
    const long long grp = u / NK;
    const int kb0 = int(u - grp * NK);
    const int kb1 = int(min<long long>(NK, kb0 + (u1 - u)));
    const int qg = int(grp % QG);
    const int head = int((grp / QG) % H);
    const int b = int(grp / ((long long)QG * H));
    const float* base = qkv + size_t(b) * T * ld;
    const int qt = qg * 4 + wv;
    const bool active = qt < QT;
    const int q0 = qt * 32;

    float qreg[32];
    {
      const int qrow = min(q0 + j, T - 1);
      const float4* qp = reinterpret_cast<const float4*>(base + size_t(qrow) * ld + head * HD + 32 * hf);
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4) {
        const float4 v = qp[s4];
        qreg[4 * s4 + 0] = v.x * scale_log2e;
        qreg[4 * s4 + 1] = v.y * scale_log2e;
        qreg[4 * s4 + 2] = v.z * scale_log2e;
        qreg[4 * s4 + 3] = v.w * scale_log2e;
      }
    }
    const float* kg = base + D + head * HD + 4 * lc4;
    const float* vg = base + 2 * D + head * HD + 4 * lc4;
    float4 pk0, pk1, pv0, pv1;
    auto fetch = [&](int blk) {
      const int r0 = min(blk * 32 + lrow, T - 1), r1 = min(blk * 32 + 16 + lrow, T - 1);
      pk0 = *reinterpret_cast<const float4*>(kg + size_t(r0) * ld);
      pk1 = *reinterpret_cast<const float4*>(kg + size_t(r1) * ld);
      pv0 = *reinterpret_cast<const float4*>(vg + size_t(r0) * ld);
      pv1 = *reinterpret_cast<const float4*>(vg + size_t(r1) * ld);
    };
    auto stash = [&](int buf) {
      *reinterpret_cast<float4*>(&lds_k[buf * KBUF + lrow * KSTR + 4 * lc4]) = pk0;
      *reinterpret_cast<float4*>(&lds_k[buf * KBUF + (16 + lrow) * KSTR + 4 * lc4]) = pk1;
      *reinterpret_cast<float4*>(&lds_v[buf * VBUF + lrow * VSTR + 4 * lc4]) = pv0;
      *reinterpret_cast<float4*>(&lds_v[buf * VBUF + (16 + lrow) * VSTR + 4 * lc4]) = pv1;
    };
    __syncthreads();  // the previous segment's last block is no longer being read
    fetch(kb0);
    stash(0);
    __syncthreads();

    f32x16 o0 = {0}, o1 = {0};
    float m = -INFINITY, l = 0.f;
    for (int blk = kb0; blk < kb1; ++blk) {
      const int buf = (blk - kb0) & 1;
      const bool more = blk + 1 < kb1;
      if (more) fetch(blk + 1);
      if (active) {
        const float* ks = &lds_k[buf * KBUF + j * KSTR + 32 * hf];
        float kreg[32];
#pragma unroll
        for (int s4 = 0; s4 < 8; ++s4) {
          const float4 v = *reinterpret_cast<const float4*>(ks + 4 * s4);
          kreg[4 * s4 + 0] = v.x;
          kreg[4 * s4 + 1] = v.y;
          kreg[4 * s4 + 2] = v.z;
          kreg[4 * s4 + 3] = v.w;
        }
        const float* vs = &lds_v[buf * VBUF + j];
        float v0[16], v1[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          v0[t] = vs[key_of(t, hf) * VSTR];
          v1[t] = vs[key_of(t, hf) * VSTR + 32];
        }
        f32x16 sacc = {0};
#pragma unroll
        for (int st = 0; st < 32; ++st) sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kreg[st], qreg[st], sacc, 0, 0, 0);
        const int kb = blk * 32;
        if (kb + 32 > T) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (kb + key_of(r, hf) >= T) sacc[r] = -INFINITY;
        }
        float mx = sacc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sacc[r]);
        mx = half_max(mx);
        const float m_new = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f(m - m_new);
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sacc[r] = __builtin_amdgcn_exp2f(sacc[r] - m_new);
          psum += sacc[r];
        }
        psum = half_sum(psum);
        l = l * alpha + psum;
        m = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          o0[r] *= alpha;
          o1[r] *= alpha;
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[t], sacc[t], o0, 0, 0, 0);
          o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[t], sacc[t], o1, 0, 0, 0);
        }
      }
      if (more) stash(buf ^ 1);
      __syncthreads();
    }

    if (active) {
      if (kb0 == 0 && kb1 == NK) {
        const int q = q0 + j;
        if (q < T) {
          const float inv = 1.f / l;
          float* orow = out + (size_t(b) * T + q) * D + head * HD;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int d = key_of(r, hf);
            orow[d] = o0[r] * inv;
            orow[32 + d] = o1[r] * inv;
          }
        }
      } else {
        // slot layout: part_o[wg][first?0:1][wave][d][32 queries], part_ml[wg][slot][wave][2][32]
        const size_t slot = (size_t(w) * 2 + (first ? 0 : 1)) * 4 + wv;
        float* po = part_o + slot * (HD * 32);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int d = key_of(r, hf);
          po[d * 32 + j] = o0[r];
          po[(32 + d) * 32 + j] = o1[r];
        }
        if (hf == 0) {
          part_ml[slot * 64 + j] = m;
          part_ml[slot * 64 + 32 + j] = l;
        }
      }
    }
    u += kb1 - kb0;
    first = false;
  }
}

}  // namespace

extern "C" {

// Resident attention waves per CU (occupancy of attn_fwd_sk); the persistent grid is this times
// the slice's CU count.
// Variant: 0 = LDS-shared K/V workgroup kernel (default); 2 / 3 = one-wave kernel with 2 or 3
// resident waves per SIMD (register budget 256 or 168 VGPRs), kept for A/B measurement.
static int g_variant = 0;

int nos_attention_set_variant(int v) {
  if (v != 0 && v != 2 && v != 3) return -1;
  g_variant = v;
  return 0;
}

// Persistent grid slots per CU for the selected variant (workgroups, not waves).
int nos_attention_waves_per_cu() {
  int n = 0;
  hipError_t e;
  if (g_variant == 0)
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, attn_fwd_sk_lds, 256, 0);
  else if (g_variant == 3)
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, attn_fwd_sk<3>, 64, 0);
  else
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, attn_fwd_sk<2>, 64, 0);
  if (e != hipSuccess || n <= 0) n = g_variant == 0 ? 2 : 4 * g_variant;
  return n;
}

// bytes of caller-provided workspace for a stream-K launch of `waves` waves. The workspace comes
// from the caller's stream-ordered allocator, so concurrent slices never share scratch and a launch
// inside graph capture never allocates.
size_t nos_attention_ws_bytes(int waves) {
  return size_t(waves) * 2 * (HD * 32 + 64) * sizeof(float) * (g_variant == 0 ? 4 : 1);
}

int nos_attention_f32_sk(const float* qkv, float* out, float* ws, int B, int T, int H, int head_dim, float scale,
                         int waves, void* stream) {
  if (head_dim != HD) {
    nos_kernels_set_error("attention: head_dim must be 64");
    return -1;
  }
  if (ws == nullptr || waves <= 0) {
    nos_kernels_set_error("attention: stream-K launch needs waves > 0 and a workspace (nos_attention_ws_bytes)");
    return -1;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float scale_log2e = scale * 1.4426950408889634f;
  const int NK = (T + 31) / 32;
  if (g_variant == 0) {
    const int QG = (NK + 3) / 4;
    float* part_o = ws;
    float* part_ml = ws + size_t(waves) * 8 * HD * 32;
    hipLaunchKernelGGL(attn_fwd_sk_lds, dim3(waves), dim3(256), 0, s, qkv, out, part_o, part_ml, B, T, H,
                       scale_log2e, waves);
    if (int rc = nos_kernels_check_launch("attn_fwd_sk_lds")) return rc;
    nos_attn_sk_lds_fixup4_launch(dim3(B * H * QG * 4), s, part_o, part_ml, out, B, T, H, waves);
    return nos_kernels_check_launch("attn_sk_lds_fixup");
  }
  float* part_o = ws;
  float* part_ml = ws + size_t(waves) * 2 * HD * 32;
  if (g_variant == 3)
    hipLaunchKernelGGL(attn_fwd_sk<3>, dim3(waves), dim3(64), 0, s, qkv, out, part_o, part_ml, B, T, H, scale_log2e,
                       waves);
  else
    hipLaunchKernelGGL(attn_fwd_sk<2>, dim3(waves), dim3(64), 0, s, qkv, out, part_o, part_ml, B, T, H, scale_log2e,
                       waves);
  if (int rc = nos_kernels_check_launch("attn_fwd_sk")) return rc;
  hipLaunchKernelGGL(attn_sk_fixup, dim3(B * H * NK), dim3(256), 0, s, part_o, part_ml, out, B, T, H, waves);
  return nos_kernels_check_launch("attn_sk_fixup");
}

int nos_attention_f32(const float* qkv, float* out, int B, int T, int H, int head_dim, float scale, void* stream) {
  if (head_dim != HD) {
    nos_kernels_set_error("attention: head_dim must be 64");
    return -1;
  }
  const int qtiles = (T + 31) / 32;
  hipLaunchKernelGGL(attn_fwd_f32, dim3(qtiles, H, B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), qkv, out,
                     T, H, scale * 1.4426950408889634f);
  return nos_kernels_check_launch("attn_fwd_f32");
}

}  // extern "C"
