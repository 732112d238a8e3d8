// Grounded decoding: the region-token grammar of the answer format `<p>phrase</p><roi><r_k>...</roi>` applied to the logits of
// one decode step, between the head GEMV and the sampler (gr_grammar_step, include/groma_hip.h; the host statement of the same
// table is groma_amd/grammar.py).  Three states per row, one contiguous id range R = [r_first, r_first + r_count), a per-row box
// count n: everything is read from device memory, so ONE captured launch serves any mix of rows and states.
//
//   state -1            the row is not constrained: the block returns before it touches anything
//   state 0  TEXT       banned: all of R, eor, the `never` ids, and bor when n == 0         (<= r_count + 2 + n_never stores)
//   state 1  OPEN       banned: everything except r_first .. r_first + n - 1 (n == 0: everything except eor)   (a row sweep)
//   state 2  BODY       banned: everything except r_first .. r_first + n - 1 and eor                           (a row sweep)
//
// The transition on the last emitted token t runs first: bor -> 1, t in R -> 2, eor -> 0, anything else (no token yet, a pad,
// an EOS) leaves the state.  A banned logit becomes -inf; allowed ones are not read and not written.  The sweep is store-only:
// consecutive lanes write consecutive floats (whole 256-byte lines per wave), 1024 threads per row.
#include "gr_common.h"

struct gr_never_ids { long id[8]; };  // by value in the launch arguments: a captured graph keeps them

__global__ __launch_bounds__(1024) void grammar_step_kernel(float* __restrict__ logits, int V, long ld, int* __restrict__ state,
                                                            const long* __restrict__ last_tok, const int* __restrict__ n_boxes,
                                                            long r_first, int r_count, long bor, long eor, gr_never_ids never,
                                                            int n_never) {
  const int row = blockIdx.x, tid = threadIdx.x;
  int s = state[row];
  if (s < 0) return;  // (uniform over the block)
  const long t = last_tok ? last_tok[row] : -1;
  if (t == bor) s = 1;
  else if (t >= r_first && t < r_first + r_count) s = 2;
  else if (t == eor) s = 0;
  __syncthreads();  // every thread has read the old state
  if (tid == 0) state[row] = s;
  const int n = min(max(n_boxes[row], 0), r_count);
  float* xr = logits + (long)row * ld;
  if (s == 0) {
    const int m = r_count + 2 + n_never;
    for (int i = tid; i < m; i += 1024) {
      long id;
      if (i < r_count) id = r_first + i;
      else if (i == r_count) id = eor;
      else if (i == r_count + 1) id = n == 0 ? bor : -1;
      else id = never.id[i - r_count - 2];
      if (id >= 0) xr[id] = -INFINITY;
    }
    return;
  }
  // OPEN / BODY: allowed = [a0, a1) and, in BODY or with no boxes, eor
  const int a0 = (int)r_first, a1 = (int)r_first + n;
  const int keep = (s != 1 || n == 0) ? (int)eor : -1;
  for (int i = tid; i < V; i += 1024)
    if ((i < a0 || i >= a1) && i != keep) xr[i] = -INFINITY;
}

extern "C" int gr_grammar_step(float* logits, int rows, int V, long ld, int* state, const long* last_tok, const int* n_boxes,
                               long r_first, int r_count, long bor, long eor, const long* never, int n_never, hipStream_t stream) {
  if (!logits || !state || !n_boxes || rows <= 0 || V <= 0 || ld < V) return GR_EINVAL;
  if (r_count < 0 || r_first < 0 || r_first > V || r_count > V - r_first) return GR_EINVAL;
  if (bor < 0 || bor >= V || eor < 0 || eor >= V || bor == eor) return GR_EINVAL;
  if ((bor >= r_first && bor < r_first + r_count) || (eor >= r_first && eor < r_first + r_count)) return GR_EINVAL;
  if (n_never < 0 || n_never > 8 || (n_never > 0 && !never)) return GR_EINVAL;
  gr_never_ids nv;
  for (int i = 0; i < 8; ++i) {
    nv.id[i] = i < n_never ? never[i] : -1;
    if (i < n_never && (nv.id[i] < 0 || nv.id[i] >= V)) return GR_EINVAL;
  }
  hipLaunchKernelGGL(grammar_step_kernel, dim3(rows), dim3(1024), 0, stream, logits, V, ld, state, last_tok, n_boxes, r_first,
                     r_count, bor, eor, nv, n_never);
  GR_CHECK_LAUNCH();
  return GR_OK;
}
