// Teacher-forced scoring: the log-probability of a GIVEN label under softmax of each logits row (gr_label_logprob_rows,
// include/groma_hip.h), with the row's log-normaliser, its arg-max and the label's rank, in ONE pass over the row -- and the row
// gather in front of the rows-only head (gr_gather_rows_f32).  Built for thousands of rows: one 256-thread workgroup per row (a
// full-size call has far more rows than the chip has CUs, and 8 workgroups fit a CU), consecutive lanes read consecutive 16-byte
// vectors, every thread keeps four loads in flight.
//
//   t = labels[row] < 0   the block returns before it touches the row: logprob = 0, lse = 0, greedy = -1, rank = -1
//   t >= V                logprob = NaN, rank = -1; lse and greedy as usual (x is never read outside [0, V))
//   otherwise             lse = m + log(sum_j exp(x[j] - m)), m = the row maximum;  logprob = x[t] - lse  (natural log, raw logits)
//                         greedy = the first maximal index (argmax_kernel's tie rule)
//                         rank   = #{j : x[j] > x[t], or x[j] == x[t] and j < t}     (0: the label is the greedy token)
//   -inf logits carry no mass; a label at -inf gives -inf; an all -inf row gives logprob = NaN, lse = -inf, greedy = 0.
//
// THE SUMMATION ORDER (fixed: results are bit-reproducible; tests/test_score_gpu.py restates it in float32 numpy).
// A UNIT is the 16-byte vector i = elements 4i .. 4i+3 (i < V / 4), or one of the V % 4 tail elements.  State: (m, s), m = -inf, s = 0.
//   unit      u = max of the unit;  if u > m: s = s * exp(m - u), m = u;  if m > -inf: s = s + exp(x[e] - m) for the unit's e in index order
//   thread    tid takes vectors tid, tid + 256, tid + 512, ... in that order, then (tid < V % 4) tail element 4 * (V / 4) + tid
//   merge     (m, s) (+) (m', s') = (M, s * f(m, M) + s' * f(m', M)),  M = max(m, m'),  f(a, M) = 0 if a = -inf else exp(a - M)
//   wave      butterfly: lane l merges with lane l ^ 32, then ^ 16, 8, 4, 2, 1 (both partners compute the same sum: + commutes)
//   block     the four wave leaders through LDS; thread 0 merges wave 0 (+) wave 1, (+) wave 2, (+) wave 3
// exp is __expf, log is logf; the file is compiled without FMA contraction (csrc/build.py), so every line above is one rounding per
// operation.  A row whose base address is not 16-byte aligned reads each vector as four scalar loads: same units, same order, same bits.
// The arg-max index and the rank count ride the same pass (x[t] is one scalar load taken before the sweep); no global atomics.
#include "gr_common.h"

#define SCORE_THREADS 256
#define SCORE_UNROLL 4

struct score_acc {
  float m, s;  // running maximum, sum of exp(x - m)
  int bi;      // first index holding m (0x7fffffff: none yet)
  int cnt;     // elements ranked before the label
};

__device__ __forceinline__ float score_f(float a, float M) { return a == -INFINITY ? 0.f : __expf(a - M); }

template <int N>
__device__ __forceinline__ void score_unit(score_acc& a, const float (&v)[N], int j0, float xt, int t) {
  float u = v[0];
#pragma unroll
  for (int e = 1; e < N; ++e) u = fmaxf(u, v[e]);
  if (u > a.m) {
    a.s = a.s * __expf(a.m - u);  // (m = -inf: s is 0 and stays 0)
    a.m = u;
    int first = N - 1;
#pragma unroll
    for (int e = N - 2; e >= 0; --e) first = v[e] == u ? e : first;
    a.bi = j0 + first;
  }
  if (a.m > -INFINITY) {
#pragma unroll
    for (int e = 0; e < N; ++e) a.s = a.s + __expf(v[e] - a.m);
  }
#pragma unroll
  for (int e = 0; e < N; ++e) a.cnt += (v[e] > xt || (v[e] == xt && j0 + e < t)) ? 1 : 0;
}

__device__ __forceinline__ void score_merge(score_acc& a, float om, float os, int obi, int ocnt) {
  const float M = fmaxf(a.m, om);
  const float mine = a.s * score_f(a.m, M), theirs = os * score_f(om, M);
  a.s = mine + theirs;
  if (om > a.m || (om == a.m && obi < a.bi)) a.bi = obi;
  a.m = M;
  a.cnt += ocnt;
}

template <bool VEC>
__device__ __forceinline__ void score_load(const float* __restrict__ xr, int i, int nv, float (&v)[4]) {
  if (i >= nv) {  // past the last whole vector: a unit of -inf adds nothing to any of the four results
    v[0] = v[1] = v[2] = v[3] = -INFINITY;
  } else if (VEC) {
    const f32x4 q = *(const f32x4*)(xr + 4 * (long)i);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
    v[0] = xr[4 * (long)i]; v[1] = xr[4 * (long)i + 1]; v[2] = xr[4 * (long)i + 2]; v[3] = xr[4 * (long)i + 3];
  }
}

template <bool VEC>
__device__ __forceinline__ void score_sweep(score_acc& a, const float* __restrict__ xr, int V, float xt, int t) {
  const int tid = threadIdx.x, nv = V >> 2;
  for (int base = tid; base < nv; base += SCORE_THREADS * SCORE_UNROLL) {
    float v[SCORE_UNROLL][4];
#pragma unroll
    for (int u = 0; u < SCORE_UNROLL; ++u) score_load<VEC>(xr, base + u * SCORE_THREADS, nv, v[u]);
#pragma unroll
    for (int u = 0; u < SCORE_UNROLL; ++u) {
      const int i = base + u * SCORE_THREADS;
      // (a unit past nv holds -inf only and sits at an index >= 4 * nv + ...: it is given j0 = V, beyond every label)
      score_unit<4>(a, v[u], i < nv ? 4 * i : V, xt, t);
    }
  }
  const int j = 4 * nv + tid;
  if (j < V) {
    const float one[1] = {xr[j]};
    score_unit<1>(a, one, j, xt, t);
  }
}

__global__ __launch_bounds__(SCORE_THREADS) void label_logprob_rows_kernel(const float* __restrict__ x, int V, long ld,
                                                                           const long* __restrict__ labels, float* __restrict__ logprob,
                                                                           float* __restrict__ lse, long* __restrict__ greedy,
                                                                           int* __restrict__ rank) {
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long t = labels[row];
  if (t < 0) {  // (uniform over the block) an ignored row: its logits are not read
    if (tid == 0) {
      logprob[row] = 0.f;
      if (lse) lse[row] = 0.f;
      if (greedy) greedy[row] = -1;
      if (rank) rank[row] = -1;
    }
    return;
  }
  const float* xr = x + (long)row * ld;
  const bool in = t < V;
  const float xt = in ? xr[t] : NAN;  // NaN compares false with everything: nothing is counted
  const int ti = in ? (int)t : V;
  score_acc a = {-INFINITY, 0.f, 0x7fffffff, 0};
  if ((((uintptr_t)xr) & 15) == 0) score_sweep<true>(a, xr, V, xt, ti);
  else score_sweep<false>(a, xr, V, xt, ti);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    score_merge(a, __shfl_xor(a.m, o, 64), __shfl_xor(a.s, o, 64), __shfl_xor(a.bi, o, 64), __shfl_xor(a.cnt, o, 64));
  __shared__ float sm[SCORE_THREADS / 64], ss[SCORE_THREADS / 64];
  __shared__ int sb[SCORE_THREADS / 64], sc[SCORE_THREADS / 64];
  if (lane == 0) { sm[wave] = a.m; ss[wave] = a.s; sb[wave] = a.bi; sc[wave] = a.cnt; }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < SCORE_THREADS / 64; ++w) score_merge(a, sm[w], ss[w], sb[w], sc[w]);
  const float l = a.m + logf(a.s);
  logprob[row] = in ? xt - l : NAN;
  if (lse) lse[row] = l;
  if (greedy) greedy[row] = a.m == -INFINITY ? 0 : a.bi;
  if (rank) rank[row] = in ? a.cnt : -1;
}

extern "C" int gr_label_logprob_rows(const float* x, int rows, int V, long ld, const long* labels, float* logprob, float* lse,
                                     long* greedy, int* rank, hipStream_t stream) {
  if (!x || !labels || !logprob || rows <= 0 || V <= 0 || ld < V) return GR_EINVAL;
  hipLaunchKernelGGL(label_logprob_rows_kernel, dim3(rows), dim3(SCORE_THREADS), 0, stream, x, V, ld, labels, logprob, lse, greedy,
                     rank);
  GR_CHECK_LAUNCH();
  return GR_OK;
}

// dst[r, :] = src[row_idx[r], :]  (fp32 rows of C % 4 == 0 columns, 16-byte vectors; the rows-only head gathers the residual rows
// that carry a label).  An index outside [0, src_rows) reads nothing and leaves zeros.
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, const int* __restrict__ row_idx,
                                                          float* __restrict__ dst, long n, int C, long src_rows) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4 = C >> 2;
  if (idx >= n * c4) return;
  const int c = (int)(idx % c4) << 2;
  const long r = idx / c4;
  const long s = row_idx[r];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (s >= 0 && s < src_rows) v = *(const f32x4*)(src + s * C + c);
  *(f32x4*)(dst + r * C + c) = v;
}
extern "C" int gr_gather_rows_f32(const float* src, const int* row_idx, float* dst, long n, int C, long src_rows, hipStream_t stream) {
  if (!src || !row_idx || !dst || C <= 0 || C % 4 != 0 || src_rows <= 0) return GR_EINVAL;
  if (n <= 0) return GR_OK;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(gr_cdiv(n * (C >> 2), 256)), dim3(256), 0, stream, src, row_idx, dst, n, C, src_rows);
  GR_CHECK_LAUNCH();
  return GR_OK;
}
