// Argument block and shared prologue / epilogue pieces of the decode-step weight-streaming kernels (gemv_fused.hip: 16-bit weights;
// gemv_fp8.hip: e4m3 weights).
#pragma once
#include "gr_common.h"
#include "kv_layout.h"

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
  // epi 3 into a paged cache (gr_gemv_fused_paged; null for gr_gemv_fused): kc / vt are the page pools, row m's block table is
  // table[m * table_ld ..] (kv_layout.h).  Appended last: the slot instantiations keep every field offset.
  const int* table;
  int table_ld;
};

// ---- the pieces both streams share.  Their weight loads, products and cross-lane reductions differ (and the shuffles stay in the
// kernels: all 64 lanes must take part); what happens around them is this, per group and per finished (row n, batch row m) element.

// row rr (0 .. ROWS-1) of a group whose two halves start at rows r_lo and r_hi
template <int ROWS>
__device__ __forceinline__ int gemv_row(int r_lo, int r_hi, int rr) { return rr < ROWS / 2 ? r_lo + rr : r_hi + (rr - ROWS / 2); }
// the two halves of group g: ROWS / 2 consecutive rows each.  epi 3 (fused QKV), inside the q and k sections: ROWS / 2 dims d of
// one head and their rotate_half partners d + HD / 2; the v section and every other mode: ROWS consecutive rows.
template <int ROWS>
__device__ __forceinline__ void gemv_group_rows(const GemvFArgs& p, int g, int& r_lo, int& r_hi) {
  r_lo = g * ROWS;
  r_hi = g * ROWS + ROWS / 2;
  if (p.epi == 3 && (long)g * ROWS < 2L * p.H * p.HD) {
    const int bph = p.HD / ROWS;  // groups per head
    const int hh = g / bph, j = g - hh * bph;
    r_lo = hh * p.HD + j * (ROWS / 2);
    r_hi = r_lo + p.HD / 2;
  }
}

// x_mode 2: elements k0 .. k0 + 7 of batch row m of the attention context, merged from decode_attention's key slices in slice order
// and rounded like its nsplit = 1 output (zero for the padding rows m >= M)
__device__ __forceinline__ bf16x8 gemv_merge8(const GemvFArgs& p, int m, int k0) {
  union { bf16x8 v; uint32_t u[4]; } pk;
  pk.v = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
  if (m < p.M) {
    const int hd = p.a_hd;
    const int hh = k0 / hd, dd = k0 - hh * hd;
    const float* base = p.a_parts + ((long)(m * (p.K / hd) + hh) * p.a_nsplit) * (hd + 2);
    float mx = -1e30f;
    for (int i = 0; i < p.a_nsplit; ++i) mx = fmaxf(mx, base[i * (hd + 2) + hd]);
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, l = 0.f;
    for (int i = 0; i < p.a_nsplit; ++i) {
      const float* bi = base + i * (hd + 2);
      const float f = __expf(bi[hd] - mx);
      l += f * bi[hd + 1];
      const f32x4 o0 = *(const f32x4*)(bi + dd), o1 = *(const f32x4*)(bi + dd + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[e] += f * o0[e]; o[4 + e] += f * o1[e]; }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)  // (every slice empty -- the row has no visible key: zeros, as gr_decode_attention's nsplit = 1 output)
      pk.u[e] = l > 0.f ? pack2bf(o[2 * e] / l, o[2 * e + 1] / l) : 0u;
  }
  return pk.v;
}

// ---- epilogue stores of one finished element y = (x . W^T)[m, n]
__device__ __forceinline__ void gemv_store_f32(const GemvFArgs& p, int m, int n, float y) { ((float*)p.C)[(long)m * p.ldc + n] = y; }  // epi 0
__device__ __forceinline__ void gemv_add_resid(const GemvFArgs& p, int m, int n, float y) { p.resid[(long)m * p.ldr + n] += y; }      // epi 1
// epi 2: interleaved rows, even n = gate_j, odd n + 1 = up_j -> out[m, j]
__device__ __forceinline__ void gemv_store_swiglu(const GemvFArgs& p, int m, int n, float gate, float up) {
  ((bf16_t*)p.C)[(long)m * p.ldc + (n >> 1)] = f2bf(silu_f(gate) * up);
}
__device__ __forceinline__ int gemv_pos(const GemvFArgs& p, int m) { return p.pos_dev ? p.pos_dev[m * p.pos_stride] : p.pos0; }
// epi 3: section (0 q / 1 k / 2 v) and head of the group whose first row is r0.  All rows of a group lie in ONE head (HD % ROWS == 0),
// so both are wave-uniform scalars -- no per-lane division.
__device__ __forceinline__ void gemv_qkv_head(const GemvFArgs& p, int r0, int& sect, int& hh) {
  const int HHD = p.H * p.HD;
  sect = r0 / HHD;
  hh = (r0 - sect * HHD) / p.HD;
}
// epi 3: row n of that group.  The projection is rounded to 16 bits first (what the prefill GEMM stores), then rotate_half in f32 with
// `partner` = the rounded value of row d -+ HD/2; K rows and V^T columns go to the slot or (PAGED) the paged cache at position pos.
template <bool PAGED>
__device__ __forceinline__ void gemv_store_qkv(const GemvFArgs& p, int m, int pos, int sect, int hh, int n, float y, float partner) {
  const int HHD = p.H * p.HD;
  const int d = n - sect * HHD - hh * p.HD;
  const int HALF = p.HD / 2;
  const long bh = (long)m * p.H + hh;
  if (sect == 2) {
    if constexpr (PAGED) p.vt[kv_vt_paged(kv_page(p.table, p.table_ld, m, pos), p.H, hh, pos, d, p.HD)] = f2bf(y);
    else p.vt[kv_vt_slot(bh, pos, d, p.HD, p.kv_stride)] = f2bf(y);
  } else {
    const float a = bf2f(f2bf(y));
    float o = a;
    if (p.cosT) {
      const int dc = d < HALF ? d : d - HALF;
      const float sgn = d < HALF ? -1.f : 1.f;
      o = a * p.cosT[(long)pos * HALF + dc] + sgn * partner * p.sinT[(long)pos * HALF + dc];
    }
    if (sect == 0) p.q[bh * p.HD + d] = f2bf(o);
    else if constexpr (PAGED) p.kc[kv_k_paged(kv_page(p.table, p.table_ld, m, pos), p.H, hh, pos, d, p.HD)] = f2bf(o);
    else p.kc[kv_k_slot(bh, pos, d, p.HD, p.kv_stride)] = f2bf(o);
  }
}

// the e4m3 stream (gemv_fp8.hip); MB = 4 | 8 batch rows staged; p.table != null: the paged epi 3
int gr_launch_gemv_fp8(const GemvFArgs& p, int MB, int n_cu, hipStream_t stream);

