// gm_edge_rows.hpp -- the row of every CSR position, computed once per call: shared by gm_components.hip and gm_spanning_forest.hip,
// whose edge kernels then read (row, column) of an edge coalesced with lane = edge, so that their balance does not depend on row
// lengths (a giant row is no special case).  The kernel is static: every unit that includes this gets its own copy.
#pragma once
#include "gm_internal.hpp"

namespace gm {

constexpr int kCcBlock = 256;   // (not measured: the block size of gm_triangles.hip)
constexpr int kCcPiece = 4096;  // edges per workgroup of k_cc_edge_rows (measured: 256 / 1024 / 4096 / 16384 took 1.16 / 0.41 / 0.30 / 0.49 ms on RMAT-22)

// the row that holds edge e: the r in [lo, hi) with rowptr[r] <= e < rowptr[r + 1] (given rowptr[lo] <= e < rowptr[hi])
__device__ __forceinline__ int cc_row_of(const int64_t* __restrict__ rowptr, int lo, int hi, int64_t e) {
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (rowptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

// A workgroup's kCcPiece consecutive edges lie in few rows: the rows of its first and last edge are searched in all of rowptr
// (the same for every lane: two chains of dependent loads, which is why a piece is more than a block's worth of edges), every
// lane then searches between the two.
static __global__ void __launch_bounds__(kCcBlock)
k_cc_edge_rows(gm_csr_t A, int32_t* __restrict__ row_of_edge) {
  const int64_t first = (int64_t)blockIdx.x * kCcPiece;
  if (first >= A.nnz) return;
  const int64_t last = first + kCcPiece - 1 < A.nnz ? first + kCcPiece - 1 : A.nnz - 1;
  const int rlo = cc_row_of(A.rowptr, 0, A.nrows, first);
  const int rhi = cc_row_of(A.rowptr, rlo, A.nrows, last);
  for (int64_t e = first + threadIdx.x; e <= last; e += kCcBlock) row_of_edge[e] = cc_row_of(A.rowptr, rlo, rhi + 1, e);
}

static inline unsigned cc_grid(int64_t n, int per_block = kCcBlock) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace gm
