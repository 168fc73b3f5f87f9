// nos workload kernels for gfx950 (MI355X): what the kernel families of libnos_kernels.so share at
// run time. The kernels themselves:
//
//  * norm.hip: LayerNorm, the split-K / stream-K combine + LayerNorm, bias + GELU, the x3 plane split;
//  * attn_x3.hip (and attn_wide.hip): fp32-accurate flash attention on the bf16 matrix cores over the
//    three-bf16-plane ("x3") form of Q/K/V — the model's path;
//  * attn_f32.hip: flash attention on the f32-input MFMA (set_fp32_matmul("f32"));
//  * gemm.hip / gemm_x3.hip / head.hip / attn_proj.hip: the GEMMs, the detection heads and the fused
//    attention projection.
//
// Here: the thread-local error string every family reports through (err.h), and the XCD pin of the
// enqueuing thread (pin.h) with its census kernel.
#include <hip/hip_runtime.h>

#include "err.h"
#include "pin.h"

#include <string>

namespace {
thread_local std::string g_err;
}  // namespace

void nos_kernels_set_error(const std::string& msg) { g_err = msg; }

int nos_kernels_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return int(e);
}

// ------------------------------------------------------------------------------------------
// Pinning census (tests/test_gpu_pin.py): every logical block of a pinned launch counts itself and
// records the XCD it ran on.
__global__ __launch_bounds__(64) void pin_census(int* __restrict__ counts, int* __restrict__ xcc, int n,
                                                 unsigned pin) {
  const PinnedBlock pb = pinned_block(pin);
  if (pb.id < 0 || pb.id >= n || threadIdx.x) return;
  atomicAdd(&counts[pb.id], 1);
  xcc[pb.id] = xcc_id();
}

extern "C" {

static thread_local unsigned g_pin = 0;  // per enqueuing thread, like the Python slice state

// XCD mask of the partition whose launches are being enqueued (0 = unpinned; pin.h). Set per slice
// before its work is enqueued or captured, like its CU count: a captured graph keeps the pin.
int nos_set_pin(unsigned mask) {
  if (mask > 0xffu) {
    g_err = "pin: XCD mask must fit 8 bits";
    return -1;
  }
  g_pin = mask;
  return 0;
}

unsigned nos_pin_mask() { return g_pin; }

int nos_pin_census(int* counts, int* xcc, int n, unsigned pin, void* stream) {
  hipLaunchKernelGGL(pin_census, dim3(pinned_grid(n, pin)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), counts,
                     xcc, n, pin);
  return nos_kernels_check_launch("pin_census");
}

const char* nos_kernels_last_error() { return g_err.c_str(); }

}  // extern "C"
