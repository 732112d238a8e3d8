// Argument block shared by the decode-step weight-streaming kernels (gemv_fused.hip: 16-bit weights; gemv_fp8.hip: e4m3 weights).
#pragma once
#include "gr_common.h"

struct GemvFArgs {
  const bf16_t* W;
  long ldw;
  int M, N, K;
  int x_mode;  // 0: A bf16 [M,K] ; 1: RMSNorm(h) * gamma ; 2: merged attention slices (a_parts)
  const bf16_t* A;
  long lda;
  const float* h;
  long ldh;
  const float* gamma;
  float eps;
  const float* a_parts;
  int a_nsplit, a_hd;
  int epi;  // 0: f32 out ; 1: resid += ; 2: SwiGLU -> bf16 [M, N/2] ; 3: QKV RoPE + cache write
  void* C;
  long ldc;
  float* resid;
  long ldr;
  bf16_t* q;
  bf16_t* kc;
  bf16_t* vt;
  const float* cosT;
  const float* sinT;
  int H, HD, pos0, kv_stride;
  const int* pos_dev;
  int pos_stride;
  const float* w_scale;  // e4m3 stream: per-output-row scale of the weight [N]
  // epi 3 into a paged cache (gr_gemv_fused_paged; null for gr_gemv_fused): kc [pages, H, 64, HD], vt [pages, H, HD, 64], row m's
  // position pos in page table[m * table_ld + pos / 64].  Appended last: the slot instantiations keep every field offset.
  const int* table;
  int table_ld;
};

// element offsets of (row m, head hh, position pos, dim d) in the paged K and V^T pools.  A position past the row's table writes into
// page 0, the pool's sink page (never handed to a request).
__device__ __forceinline__ long gf_page(const GemvFArgs& p, int m, int pos) {
  const int i = pos >> 6;
  return (unsigned)i < (unsigned)p.table_ld ? (long)p.table[(long)m * p.table_ld + i] : 0L;
}
__device__ __forceinline__ long gf_k_page_off(const GemvFArgs& p, int m, int hh, int pos, int d) {
  return ((gf_page(p, m, pos) * p.H + hh) * 64 + (pos & 63)) * p.HD + d;
}
__device__ __forceinline__ long gf_vt_page_off(const GemvFArgs& p, int m, int hh, int pos, int d) {
  return ((gf_page(p, m, pos) * p.H + hh) * p.HD + d) * 64 + (pos & 63);
}

// the e4m3 stream (gemv_fp8.hip); MB = 4 | 8 batch rows staged; p.table != null: the paged epi 3
int gr_launch_gemv_fp8(const GemvFArgs& p, int MB, int n_cu, hipStream_t stream);

