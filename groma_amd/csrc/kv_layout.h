// The two layouts of the decode KV cache: one formula each, used by every kernel that reads or writes the cache.
//   slot : k [rows, H, kv_stride, HD] (one K row per position), vt [rows, H, HD, kv_stride] (V transposed: one column per position)
//   paged: k [pages, H, KV_PAGE, HD], vt [pages, H, HD, KV_PAGE]; position pos of row b lies in page table[b * table_ld + pos / KV_PAGE]
//          at offset pos % KV_PAGE.  A position past the row's table maps to page 0, the pool's sink page (never handed to a request).
// bh = row * H + head.  Offsets are in (logical) elements.
#pragma once
#include "gr_common.h"

#define KV_PAGE_SHIFT 6
#define KV_PAGE (1 << KV_PAGE_SHIFT)  // positions per page

// index of the page-table entry that holds position pos
__device__ __host__ __forceinline__ int kv_page_idx(int pos) { return pos >> KV_PAGE_SHIFT; }
// the page that holds position pos of row b
__device__ __forceinline__ long kv_page(const int* table, int table_ld, int b, int pos) {
  const int i = kv_page_idx(pos);
  return (unsigned)i < (unsigned)table_ld ? (long)table[(long)b * table_ld + i] : 0L;
}

// slot layout: element d of the K row, and the V^T element of dim d, at position pos
__device__ __forceinline__ long kv_k_slot(long bh, int pos, int d, int HD, int kv_stride) { return (bh * kv_stride + pos) * HD + d; }
__device__ __forceinline__ long kv_vt_slot(long bh, int pos, int d, int HD, int kv_stride) { return (bh * HD + d) * kv_stride + pos; }

// paged layout: the same two elements in page `page` (head h of H)
__device__ __forceinline__ long kv_k_paged(long page, int H, int h, int pos, int d, int HD) {
  return ((page * H + h) * KV_PAGE + (pos & (KV_PAGE - 1))) * HD + d;
}
__device__ __forceinline__ long kv_vt_paged(long page, int H, int h, int pos, int d, int HD) {
  return ((page * H + h) * HD + d) * KV_PAGE + (pos & (KV_PAGE - 1));
}
