// nos workload kernels for gfx950 (MI355X): the elementwise and row kernels of the fp32 YOLOS-small
// workload.
//
//  * layernorm_f32: two rows per wave in flight, values kept in registers (two-pass mean/variance), wave64
//    shuffles; writes fp32 or the x3 planes the next GEMM consumes.
//  * splitk_layernorm_f32: the split-K / stream-K GEMM's combine, residuals and LayerNorm in one pass.
//  * bias_gelu_f32: in-place exact (erf) GELU(y + b) epilogue, dwordx4 vectorised.
//  * split3_f32: fp32 -> the three bf16 planes of the x3 format (attn_x3.hip "fp32 as three bf16 planes").
#include <hip/hip_runtime.h>

#include "err.h"
#include "pin.h"
#include "streamk.h"
#include "x3_common.h"

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------
// LayerNorm (output fp32 y, or x3 planes yp with plane stride rows*D when yp != nullptr). Lane l
// owns the column pairs (2l + 128i, 2l + 128i + 1): 8-B loads, and packed 4-B bf16-pair stores per
// plane on the x3 path. R rows per wave per iteration, all R loaded before any is reduced: a slice
// sharing the GPU runs a few waves per CU over many rows each, and each iteration is one memory
// round trip, so R rows in flight cut the round trips per wave by R.
template <int NPL, int R>
__global__ __launch_bounds__(256) void layernorm_f32(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ b, float* __restrict__ y,
                                                     __bf16* __restrict__ yp, int rows, float eps, unsigned pin) {
  static_assert(NPL % 2 == 0, "hidden size must be a multiple of 128");
  const PinnedBlock pb = pinned_block(pin);
  if (pb.id < 0) return;
  constexpr int D = NPL * 64, NP = NPL / 2;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float2* w2 = reinterpret_cast<const float2*>(w);
  const float2* b2 = reinterpret_cast<const float2*>(b);
  const size_t plane2 = size_t(rows) * D / 2;  // plane stride in bf16 pairs
  // grid-stride over rows: a slice sharing the GPU launches a few workgroups per CU instead of one
  // per 4R rows (workgroup dispatch is what concurrent partitions contend for)
  const int stride = pb.n * 4;
  for (int row0 = pb.id * 4 + wave; row0 < rows; row0 += R * stride) {
    float2 v[R][NP];
    float mean[R], rstd[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      // rows past the end re-read the last row (in bounds) and are never stored
      const float2* xr = reinterpret_cast<const float2*>(x + size_t(min(row0 + k * stride, rows - 1)) * D);
#pragma unroll
      for (int i = 0; i < NP; ++i) v[k][i] = xr[i * 64 + lane];
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NP; ++i) s += v[k][i].x + v[k][i].y;
      mean[k] = wave_sum(s) * (1.0f / D);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        v[k][i].x -= mean[k];
        v[k][i].y -= mean[k];
        q += v[k][i].x * v[k][i].x + v[k][i].y * v[k][i].y;
      }
      rstd[k] = rsqrtf(wave_sum(q) * (1.0f / D) + eps);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int row = row0 + k * stride;
      if (row >= rows) break;
      if (yp) {
        uint32_t* dst = reinterpret_cast<uint32_t*>(yp) + size_t(row) * (D / 2);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const int c2 = i * 64 + lane;
          const float2 ww = w2[c2], bb = b2[c2];
          const f32x2 val = {v[k][i].x * rstd[k] * ww.x + bb.x, v[k][i].y * rstd[k] * ww.y + bb.y};
          bf16x2 h0, h1, h2;
          split3(val, h0, h1, h2);
          dst[c2] = __builtin_bit_cast(uint32_t, h0);
          dst[plane2 + c2] = __builtin_bit_cast(uint32_t, h1);
          dst[2 * plane2 + c2] = __builtin_bit_cast(uint32_t, h2);
        }
      } else {
        float2* yr = reinterpret_cast<float2*>(y + size_t(row) * D);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const int c2 = i * 64 + lane;
          const float2 ww = w2[c2], bb = b2[c2];
          yr[c2] = make_float2(v[k][i].x * rstd[k] * ww.x + bb.x, v[k][i].y * rstd[k] * ww.y + bb.y);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Split-K combine + residuals + LayerNorm: x = (part_0 + ... + part_{S-1}) + bias + res (+ r2[row %
// r2_rows]) — the split-K GEMM's epilogue, in the same order as the fused one — stored as the fp32
// residual stream xout, and, when w is given, LayerNorm(x) stored as x3 planes yp (the next GEMM's
// operand). One wave per row, grid-stride, lanes on column pairs as layernorm_f32.
template <int NPL>
__global__ __launch_bounds__(256) void splitk_layernorm_f32(const float* __restrict__ part, int splits, SkMap sk,
                                                            const float* __restrict__ bias,
                                                            const float* __restrict__ res,
                                                            const float* __restrict__ r2, int r2_rows,
                                                            float* __restrict__ xout, const float* __restrict__ w,
                                                            const float* __restrict__ b, __bf16* __restrict__ yp,
                                                            int rows, float eps, unsigned pin) {
  constexpr int D = NPL * 64, NP = NPL / 2;
  const PinnedBlock pb = pinned_block(pin);
  if (pb.id < 0) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t pstride = size_t(rows) * (D / 2);  // partial plane stride in float2
  const float2* p2 = reinterpret_cast<const float2*>(part);
  const float2* bias2 = reinterpret_cast<const float2*>(bias);
  for (int row = pb.id * 4 + wave; row < rows; row += pb.n * 4) {
    const size_t r2i = size_t(row) * (D / 2);
    float2 v[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) v[i] = p2[r2i + i * 64 + lane];
    if (sk.P > 0) {
      // stream-K partials: tile t of this row and column pair holds sk_segments(t) planes
      int ns[NP], most = 1;
      const int tr = (row / sk.bm) * sk.tiles_n;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        ns[i] = sk_segments(tr + (2 * (i * 64 + lane)) / sk.bn, sk);
        most = max(most, ns[i]);
      }
      for (int sp = 1; sp < most; ++sp) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          if (sp < ns[i]) {
            const float2 q = p2[sp * pstride + r2i + i * 64 + lane];
            v[i].x += q.x;
            v[i].y += q.y;
          }
        }
      }
    }
    for (int sp = 1; sp < splits; ++sp) {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const float2 q = p2[sp * pstride + r2i + i * 64 + lane];
        v[i].x += q.x;
        v[i].y += q.y;
      }
    }
    const float2* rr = reinterpret_cast<const float2*>(res) + r2i;
    const float2* rr2 = r2 ? reinterpret_cast<const float2*>(r2) + size_t(row % r2_rows) * (D / 2) : nullptr;
    float2* xo = reinterpret_cast<float2*>(xout) + r2i;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int c2 = i * 64 + lane;
      const float2 bb = bias2[c2], r = rr[c2];
      v[i].x = v[i].x + bb.x + r.x;
      v[i].y = v[i].y + bb.y + r.y;
      if (rr2) {
        const float2 q = rr2[c2];
        v[i].x += q.x;
        v[i].y += q.y;
      }
      xo[c2] = v[i];
      s += v[i].x + v[i].y;
    }
    if (!w) continue;
    const float mean = wave_sum(s) * (1.0f / D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      v[i].x -= mean;
      v[i].y -= mean;
      q += v[i].x * v[i].x + v[i].y * v[i].y;
    }
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / D) + eps);
    const float2* w2 = reinterpret_cast<const float2*>(w);
    const float2* b2 = reinterpret_cast<const float2*>(b);
    const size_t plane2 = size_t(rows) * D / 2;
    uint32_t* dst = reinterpret_cast<uint32_t*>(yp) + r2i;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int c2 = i * 64 + lane;
      const float2 ww = w2[c2], bb = b2[c2];
      const f32x2 val = {v[i].x * rstd * ww.x + bb.x, v[i].y * rstd * ww.y + bb.y};
      bf16x2 h0, h1, h2;
      split3(val, h0, h1, h2);
      dst[c2] = __builtin_bit_cast(uint32_t, h0);
      dst[plane2 + c2] = __builtin_bit_cast(uint32_t, h1);
      dst[2 * plane2 + c2] = __builtin_bit_cast(uint32_t, h2);
    }
  }
}

// ------------------------------------------------------------------------------------------
// bias + exact GELU, in place
__global__ __launch_bounds__(256) void bias_gelu_f32(float* __restrict__ y, const float* __restrict__ b, size_t n4,
                                                     int N4) {
  size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
  const size_t stride = size_t(gridDim.x) * 256;
  float4* y4 = reinterpret_cast<float4*>(y);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  for (; i < n4; i += stride) {
    float4 v = y4[i];
    const float4 bb = b4[i % N4];
    v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w;
    v.x = 0.5f * v.x * (1.f + erff(v.x * 0.70710678118654752f));
    v.y = 0.5f * v.y * (1.f + erff(v.y * 0.70710678118654752f));
    v.z = 0.5f * v.z * (1.f + erff(v.z * 0.70710678118654752f));
    v.w = 0.5f * v.w * (1.f + erff(v.w * 0.70710678118654752f));
    y4[i] = v;
  }
}

// fp32 [n] -> bf16 planes [3][n] (plane stride n); 4 elements per thread
__global__ __launch_bounds__(256) void split3_f32(const float* __restrict__ x, __bf16* __restrict__ y, size_t n4,
                                                  unsigned pin) {
  const PinnedBlock pb = pinned_block(pin);
  if (pb.id < 0) return;
  const size_t stride = size_t(pb.n) * 256;
  for (size_t i = size_t(pb.id) * 256 + threadIdx.x; i < n4; i += stride) {
    const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
    bf16x4 p0, p1, p2;
    split3(v, p0, p1, p2);
    reinterpret_cast<bf16x4*>(y)[i] = p0;
    reinterpret_cast<bf16x4*>(y)[n4 + i] = p1;
    reinterpret_cast<bf16x4*>(y)[2 * n4 + i] = p2;
  }
}

}  // namespace

extern "C" {

// fp32 [n] -> three bf16 planes [3][n]; n % 4 == 0
int nos_split3_f32(const float* x, void* planes, size_t n, void* stream) {
  if (n % 4) {
    nos_kernels_set_error("split3: n must be a multiple of 4");
    return -1;
  }
  const size_t n4 = n / 4;
  const int grid = int(std::min<size_t>((n4 + 255) / 256, 4096));
  const unsigned pin = nos_pin_mask();
  hipLaunchKernelGGL(split3_f32, dim3(pinned_grid(pinned_cap(grid, pin), pin)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, reinterpret_cast<__bf16*>(planes), n4, pin);
  return nos_kernels_check_launch("split3_f32");
}

// y (fp32) or yp (x3 planes [3][rows][D]) — exactly one of them non-null; `wgs` workgroups of 4
// rows each (grid-stride), 0 = one per 4 rows
int nos_layernorm_f32_grid(const float* x, const float* w, const float* b, float* y, void* yp, int rows, int D,
                           float eps, int wgs, void* stream) {
  if ((y == nullptr) == (yp == nullptr)) {
    nos_kernels_set_error("layernorm: exactly one of y / yp");
    return -1;
  }
  if (rows <= 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // rows in flight per wave (NOS_LN_ROWS, 1 or 2; read once)
  static const int R = [] {
    const char* e = std::getenv("NOS_LN_ROWS");
    return (e && std::atoi(e) == 1) ? 1 : 2;
  }();
  const int full = (rows + 4 * R - 1) / (4 * R);
  const unsigned pin = nos_pin_mask();
  const dim3 grid(pinned_grid(pinned_cap(wgs > 0 ? std::min(wgs, full) : full, pin), pin)), block(256);
  __bf16* p = reinterpret_cast<__bf16*>(yp);
#define NOS_LN_CASE(DD, NPL)                                                                      \
  case DD:                                                                                        \
    if (R == 2)                                                                                   \
      hipLaunchKernelGGL((layernorm_f32<NPL, 2>), grid, block, 0, s, x, w, b, y, p, rows, eps, pin); \
    else                                                                                          \
      hipLaunchKernelGGL((layernorm_f32<NPL, 1>), grid, block, 0, s, x, w, b, y, p, rows, eps, pin); \
    break;
  switch (D) {
    NOS_LN_CASE(384, 6)
    NOS_LN_CASE(768, 12)
    NOS_LN_CASE(1024, 16)
    NOS_LN_CASE(1536, 24)
    NOS_LN_CASE(2048, 32)
    default:
      nos_kernels_set_error("layernorm: unsupported hidden size " + std::to_string(D));
      return -1;
  }
#undef NOS_LN_CASE
  return nos_kernels_check_launch("layernorm_f32");
}

// Split-K combine (+ bias, residual, broadcast residual r2 or null) into xout, and LayerNorm(xout) as
// x3 planes into yp when w/b/yp are given; part = [splits][rows][D] fp32; D in {384, 768}; `wgs`
// workgroups of 4 rows (grid-stride), 0 = one per 4 rows.
static int splitk_layernorm(const float* part, int splits, SkMap sk, const float* bias, const float* res,
                            const float* r2, int r2_rows, float* xout, const float* w, const float* b, void* yp,
                            int rows, int D, float eps, int wgs, void* stream) {
  if (!part || splits < 1 || !bias || !res || !xout || (r2 && r2_rows <= 0) || ((w == nullptr) != (yp == nullptr)) ||
      ((w == nullptr) != (b == nullptr))) {
    nos_kernels_set_error("splitk_layernorm: partials, bias, residual and output required; LayerNorm needs w, b and yp");
    return -1;
  }
  if (rows <= 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int full = (rows + 3) / 4;
  const unsigned pin = nos_pin_mask();
  const dim3 grid(pinned_grid(pinned_cap(wgs > 0 ? std::min(wgs, full) : full, pin), pin)), block(256);
  __bf16* p = reinterpret_cast<__bf16*>(yp);
  switch (D) {
    case 384:
      hipLaunchKernelGGL(splitk_layernorm_f32<6>, grid, block, 0, s, part, splits, sk, bias, res, r2, r2_rows, xout, w,
                         b, p, rows, eps, pin);
      break;
    case 768:
      hipLaunchKernelGGL(splitk_layernorm_f32<12>, grid, block, 0, s, part, splits, sk, bias, res, r2, r2_rows, xout, w,
                         b, p, rows, eps, pin);
      break;
    default:
      nos_kernels_set_error("splitk_layernorm: unsupported hidden size " + std::to_string(D));
      return -1;
  }
  return nos_kernels_check_launch("splitk_layernorm_f32");
}

int nos_splitk_layernorm_f32(const float* part, int splits, const float* bias, const float* res, const float* r2,
                             int r2_rows, float* xout, const float* w, const float* b, void* yp, int rows, int D,
                             float eps, int wgs, void* stream) {
  return splitk_layernorm(part, splits, SkMap{0, 0, 0, 1, 1, 1}, bias, res, r2, r2_rows, xout, w, b, yp, rows, D, eps,
                          wgs, stream);
}

// The same over stream-K partials (gemm_x3k): map = {P, U, nk, bm, bn, tiles_n} from
// nos_gemm_x3_streamk_map; tile t's planes 0 .. sk_segments(t)-1 are added in order.
int nos_streamk_layernorm_f32(const float* part, const int* map, const float* bias, const float* res, const float* r2,
                              int r2_rows, float* xout, const float* w, const float* b, void* yp, int rows, int D,
                              float eps, int wgs, void* stream) {
  if (!map || map[0] <= 0 || map[1] < map[0] || map[2] <= 0 || map[3] <= 0 || map[4] <= 0 || map[4] % 2 ||
      map[5] * map[4] != D) {
    nos_kernels_set_error("streamk_layernorm: map must be {P <= U, U, nk, bm, bn (even), tiles_n} with tiles_n * bn = D");
    return -1;
  }
  return splitk_layernorm(part, 1, SkMap{map[0], map[1], map[2], map[3], map[4], map[5]}, bias, res, r2, r2_rows,
                          xout, w, b, yp, rows, D, eps, wgs, stream);
}

int nos_bias_gelu_f32(float* y, const float* b, int rows, int N, void* stream) {
  if (N % 4) {
    nos_kernels_set_error("bias_gelu: N must be a multiple of 4");
    return -1;
  }
  const size_t n4 = size_t(rows) * N / 4;
  const int grid = int(std::min<size_t>((n4 + 255) / 256, 2048));
  hipLaunchKernelGGL(bias_gelu_f32, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), y, b, n4, N / 4);
  return nos_kernels_check_launch("bias_gelu_f32");
}

}  // extern "C"
