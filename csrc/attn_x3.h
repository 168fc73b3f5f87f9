// Launch descriptor of the x3 attention (attn_x3.hip): one struct, one entry point. A new launch
// parameter is a new field here, in walkai_nos_amd/ops/kernels.py's NosAttnX3 and in the launcher.
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct NosAttnX3 {
  int size;             // sizeof(NosAttnX3): checked first, a mismatch is an error
  int f32in;            // qkv is fp32 [B, T, 3*H*64] (split in the kernel); 0: its x3 planes (bf16)
  const void* qkv;
  size_t plane_stride;  // elements between the planes of qkv; ignored when f32in
  float* out;           // fp32 [B, Tq, H*64], or
  void* outp;           // its x3 planes [3][B*Tq*H*64]: exactly one of the two
  float* ws;            // stream-K partials: waves * 2 * (64*32 + 64) * group floats
  int* cnt;             // in-kernel merge (the wide kernel): ncnt >= B*hn*ceil(ceil(T/32)/8) row counters,
  int ncnt;             // zero before the first launch and left zero; null: the separate fixup launch
  int fixup;            // 0: leave split tiles' partials in ws for the consumer (attn_proj.hip); needs out
  int B, T, H;
  int h0, hn;           // the heads of this launch: h0 .. h0+hn-1
  int head_dim;         // 64
  float scale;
  int waves;            // persistent grid (workgroups)
  int q0, Tq;           // query window: rows q0 .. q0+Tq-1 of the T rows (0, T: all of them)
} NosAttnX3;

int nos_attention_x3(const NosAttnX3* a, void* stream);

#ifdef __cplusplus
}
#endif
