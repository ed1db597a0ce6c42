// gm_triangles.hip -- triangle counting (what the reference's src/TriangleCounting.cpp computes), exact integers.
//
// out(v) = the sorted multiset of the destinations of v's edges (duplicates and self-loops kept as given),
// c(u, v) = sum over x of min(multiplicity of x in out(u), multiplicity of x in out(v)) -- what a two-pointer merge counts --
// triangles[v] = sum over the edges u -> v (each duplicate counted) of c(u, v).
//
// Which adjacency is which: the GM_DIR_IN CSR has rows = sources, so its row v IS out(v); the GM_DIR_OUT CSR has rows =
// destinations, so its row v lists the u of the edges u -> v.  The count kernels walk the OUT adjacency's rows and intersect lists
// taken from the IN adjacency.
//
// Keys.  colidx holds DEVICE ids in ascending NATIVE column order, so the device ids of a row are not a sort order; an
// intersection needs both lists in one total order.  The keys pass (the counterpart of the reference's GetNeighbors) writes
// key[e] = native id of colidx[e] for every edge of the IN adjacency: every row ascending, duplicates adjacent.  It also finds out
// whether any row holds two equal keys.  If one does, a second pass writes 64-bit keys (native id << 32) | occurrence index (the
// position minus the first position of the run of equal ids): sum over x of min(m1, m2) is the plain SET intersection of the pairs
// (x, j), so with either key every list is strictly increasing, the kernels only ever intersect sets, and a binary search is exact.
//
// Two count kernels, both templated on the key type; a work item is one edge u -> v, B = keys(v), A = keys(u):
//   k_tc_rows    row-stationary: a wave per OUT row v stages B in LDS; groups of kTcGroup lanes take one in-edge each, stride over A
//                and binary-search B in LDS (A much longer than B: stride over B, search A in global memory); one plain store of
//                triangles[v];
//   k_tc_pieces  a row's in-edges cut into pieces of kTcPiece: a workgroup per piece, a wave per edge, both lists in global memory, the
//                elements of the shorter searched in the longer; one atomicAdd per wave into triangles[v], which the plan kernel
//                has zeroed.  It takes what k_tc_rows cannot hold (B beyond a wave's LDS share) or balance (giant rows, long rows).
//                (The pieces are this file's own: measured, 64-edge pieces beat the GM_GIANT_CHUNK-edge pieces of
//                gm_csr_t.gchunk_* by 1.5x -- one wave's chain of long searches is what bounds a call.)
// k_tc_plan deals the rows to the two kernels once per call and cuts the pieces.  Option "tc_form": 1 = k_tc_rows wherever B can be
// staged, 2 = k_tc_pieces only, 0 = automatic.  Measured on RMAT-18 .. 22 (profiles/triangle_counting.md), the pieces kernel alone
// was at least as fast as every split by the number of in-edges that was tried (k_tc_rows for rows of up to 16 .. 4096 in-edges: a
// skewed graph's work sits in rows one wave is too slow for, and the rest is within the noise), so the automatic form deals every
// row to k_tc_pieces as well; k_tc_rows stays as the form to measure against.  The counts are integers: no order of summation
// changes them.
// No kernel waits for another wave or workgroup, and every loop is bounded by a length read from rowptr.
// Measurements and the thresholds taken from them: profiles/triangle_counting.md.
#include <string.h>

#include "gm_internal.hpp"

namespace gm {

// gm_set_option("tc_form", 0 | 1 | 2): how the rows are dealt to the two count kernels (results do not depend on it)
int g_tc_form = GM_TC_FORM_DEFAULT;

constexpr int kTcBlock = 256;
constexpr int kTcWaves = kTcBlock / 64;
constexpr int kTcLdsBytes = 8192;  // a wave's LDS share in k_tc_rows: B of up to 2048 32-bit / 1024 64-bit keys (32 KB a workgroup)
constexpr int kTcGroup = 16;       // lanes that share one in-edge in k_tc_rows
constexpr int kTcSwap = 4;         // k_tc_rows searches A in global memory instead of B in LDS once |A| > kTcSwap * |B|
constexpr int kTcPiece = 64;       // in-edges per piece (a workgroup) of k_tc_pieces
static_assert(kTcWaves * kTcLdsBytes <= 65536, "static LDS per workgroup");
static_assert(64 % kTcGroup == 0, "whole groups per wave");

struct TcFlags {        // workspace slot GM_WS_TC_FLAG
  uint32_t duplicates;  // some row of the IN adjacency holds two equal keys
  uint32_t npieces;
  unsigned long long total;
};

// the wave's LDS accesses before and after stay on their sides (LDS is in order per wave)
__device__ __forceinline__ void tc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ unsigned long long tc_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// first edge of the row that holds edge e: rowptr[r] for the r with rowptr[r] <= e < rowptr[r + 1] (0 <= e < rowptr[nrows])
__device__ __forceinline__ int64_t tc_row_start(const int64_t* __restrict__ rowptr, int nrows, int64_t e) {
  int lo = 0, hi = nrows;  // the answer's r lies in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (rowptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  return rowptr[lo];
}
// is x in the strictly increasing list[0, n)?
template <class KT, class LIST>
__device__ __forceinline__ unsigned tc_find(LIST list, int64_t n, KT x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (list[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && list[lo] == x) ? 1u : 0u;
}

// ---------------- the keys ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t tc_native(const int32_t* __restrict__ native_of_dev, int32_t dev) {
  return (uint32_t)(native_of_dev ? native_of_dev[dev] : dev);
}
__global__ void __launch_bounds__(kTcBlock)
k_tc_keys32(gm_csr_t I, const int32_t* __restrict__ native_of_dev, uint32_t* __restrict__ key, TcFlags* __restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * kTcBlock + threadIdx.x;
  if (e >= I.nnz) return;
  const uint32_t k = tc_native(native_of_dev, I.colidx[e]);
  key[e] = k;
  // equal neighbours are rare without duplicate edges (the end of one row against the start of the next): only they look their row up
  if (e > 0 && tc_native(native_of_dev, I.colidx[e - 1]) == k && tc_row_start(I.rowptr, I.nrows, e) < e) flags->duplicates = 1u;
}
__global__ void __launch_bounds__(kTcBlock)
k_tc_keys64(gm_csr_t I, const uint32_t* __restrict__ key32, uint64_t* __restrict__ key) {
  const int64_t e = (int64_t)blockIdx.x * kTcBlock + threadIdx.x;
  if (e >= I.nnz) return;
  const uint32_t k = key32[e];
  int64_t first = e;
  if (e > 0 && key32[e - 1] == k) {
    const int64_t start = tc_row_start(I.rowptr, I.nrows, e);
    while (first > start && key32[first - 1] == k) first--;
  }
  key[e] = ((uint64_t)k << 32) | (uint64_t)(e - first);
}

// ---------------- the plan ------------------------------------------------------------------------------------------------
// cls[v]: 0 = k_tc_rows stores triangles[v]; 1 = triangles[v] is zeroed here and k_tc_pieces adds to it
__global__ void __launch_bounds__(kTcBlock)
k_tc_plan(gm_csr_t O, gm_csr_t I, int form, int lds_keys, unsigned char* __restrict__ cls, int32_t* __restrict__ piece_row,
          int64_t* __restrict__ piece_edge, TcFlags* __restrict__ flags, int64_t* __restrict__ triangles) {
  const int v = blockIdx.x * kTcBlock + threadIdx.x;
  if (v >= O.nrows) return;
  const int64_t e0 = O.rowptr[v], nin = O.rowptr[v + 1] - e0;
  const int64_t nb = I.rowptr[v + 1] - I.rowptr[v];
  bool pieces = nb > lds_keys;                                           // B cannot be staged
  if (form != 1) pieces = true;                                          // (tc_form 0 is 2 for now: see the head of this file)
  cls[v] = pieces ? 1 : 0;
  if (!pieces) return;
  triangles[v] = 0;
  if (nin == 0 || nb == 0) return;
  const uint32_t n = (uint32_t)((nin + kTcPiece - 1) / kTcPiece);
  const uint32_t base = atomicAdd(&flags->npieces, n);  // (a place in the list; nobody waits for it)
  for (uint32_t k = 0; k < n; k++) {
    piece_row[base + k] = v;
    piece_edge[base + k] = e0 + (int64_t)k * kTcPiece;
  }
}

// ---------------- the count kernels ---------------------------------------------------------------------------------------
template <class KT>
__global__ void __launch_bounds__(kTcBlock)
k_tc_rows(gm_csr_t O, gm_csr_t I, const KT* __restrict__ key, const unsigned char* __restrict__ cls, int64_t* __restrict__ triangles) {
  constexpr int CAP = kTcLdsBytes / (int)sizeof(KT);
  __shared__ KT s_b[kTcWaves][CAP];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int v = blockIdx.x * kTcWaves + wv;
  if (v >= O.nrows || cls[v]) return;
  const int64_t b0 = I.rowptr[v], nb = I.rowptr[v + 1] - b0;
  const int64_t e0 = O.rowptr[v], e1 = O.rowptr[v + 1];
  unsigned long long count = 0;
  if (nb > 0 && nb <= CAP && e1 > e0) {
    KT* B = s_b[wv];
    for (int64_t i = lane; i < nb; i += 64) B[i] = key[b0 + i];
    tc_wave_sync();
    const int grp = lane / kTcGroup, gl = lane % kTcGroup;
    for (int64_t p = e0 + grp; p < e1; p += 64 / kTcGroup) {
      const int u = O.colidx[p];
      const int64_t a0 = I.rowptr[u], na = I.rowptr[u + 1] - a0;
      const KT* A = key + a0;
      if (na > kTcSwap * nb) {
        for (int64_t i = gl; i < nb; i += kTcGroup) count += tc_find<KT>(A, na, B[i]);
      } else {
        for (int64_t i = gl; i < na; i += kTcGroup) count += tc_find<KT>(B, nb, A[i]);
      }
    }
  }
  count = tc_wave_sum(count);
  if (lane == 0) triangles[v] = (int64_t)count;
}

template <class KT>
__global__ void __launch_bounds__(kTcBlock)
k_tc_pieces(gm_csr_t O, gm_csr_t I, const KT* __restrict__ key, const int32_t* __restrict__ piece_row, const int64_t* __restrict__ piece_edge,
            const TcFlags* __restrict__ flags, int64_t* __restrict__ triangles) {
  if (blockIdx.x >= flags->npieces) return;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int v = piece_row[blockIdx.x];
  const int64_t p0 = piece_edge[blockIdx.x], row_end = O.rowptr[v + 1];
  const int64_t p1 = p0 + kTcPiece < row_end ? p0 + kTcPiece : row_end;
  const int64_t b0 = I.rowptr[v], nb = I.rowptr[v + 1] - b0;
  const KT* B = key + b0;
  unsigned long long count = 0;
  for (int64_t p = p0 + wv; p < p1; p += kTcWaves) {
    const int u = O.colidx[p];
    const int64_t a0 = I.rowptr[u], na = I.rowptr[u + 1] - a0;
    const KT* A = key + a0;
    if (na <= nb) {
      for (int64_t i = lane; i < na; i += 64) count += tc_find<KT>(B, nb, A[i]);
    } else {
      for (int64_t i = lane; i < nb; i += 64) count += tc_find<KT>(A, na, B[i]);
    }
  }
  count = tc_wave_sum(count);
  if (lane == 0 && count) atomicAdd(reinterpret_cast<unsigned long long*>(triangles + v), count);
}

__global__ void __launch_bounds__(kTcBlock)
k_tc_total(const int64_t* __restrict__ triangles, int n, TcFlags* __restrict__ flags) {
  __shared__ unsigned long long s_w[kTcWaves];
  unsigned long long a = 0;
  for (int64_t i = (int64_t)blockIdx.x * kTcBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTcBlock) a += (unsigned long long)triangles[i];
  a = tc_wave_sum(a);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kTcWaves; w++) a += s_w[w];
    if (a) atomicAdd(&flags->total, a);
  }
}

static inline unsigned tc_grid(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

template <class KT>
static int tc_count(gm_graph_t* g, const KT* key, unsigned char* cls, int32_t* piece_row, int64_t* piece_edge, TcFlags* flags, int64_t* d_triangles,
                    hipStream_t s) {
  const gm_csr_t &O = g->out.view, &I = g->in.view;
  const int n = O.nrows, form = g_tc_form;
  hipLaunchKernelGGL(k_tc_plan, dim3(tc_grid(n, kTcBlock)), dim3(kTcBlock), 0, s, O, I, form, kTcLdsBytes / (int)sizeof(KT), cls, piece_row, piece_edge,
                     flags, d_triangles);
  uint32_t npieces = 0;
  GM_TRY_HIP(hipMemcpyAsync(&npieces, &flags->npieces, 4, hipMemcpyDeviceToHost, s));
  GM_TRY_HIP(hipStreamSynchronize(s));
  if (form == 1) hipLaunchKernelGGL((k_tc_rows<KT>), dim3(tc_grid(n, kTcWaves)), dim3(kTcBlock), 0, s, O, I, key, (const unsigned char*)cls, d_triangles);
  if (npieces > 0)
    hipLaunchKernelGGL((k_tc_pieces<KT>), dim3(npieces), dim3(kTcBlock), 0, s, O, I, key, (const int32_t*)piece_row, (const int64_t*)piece_edge,
                       (const TcFlags*)flags, d_triangles);
  GM_TRY_HIP(hipGetLastError());
  return GM_OK;
}

static int run_triangle_count(gm_graph_t* g, int64_t* d_triangles, uint64_t* h_total, hipStream_t s) {
  const gm_csr_t& I = g->in.view;
  const int n = g->out.view.nrows;
  const int64_t nnz = I.nnz;
  int rc;
  void* p = nullptr;
  if ((rc = gm_graph_workspace(g, GM_WS_TC_FLAG, 64, &p))) return rc;
  TcFlags* flags = (TcFlags*)p;
  const size_t cls_bytes = ((size_t)n + 63) / 64 * 64, max_pieces = (size_t)n + (size_t)(g->out.view.nnz / kTcPiece) + 1;
  if ((rc = gm_graph_workspace(g, GM_WS_TC_PLAN, cls_bytes + 64 + max_pieces * 12, &p))) return rc;
  unsigned char* cls = (unsigned char*)p;
  int64_t* piece_edge = (int64_t*)(cls + cls_bytes);
  int32_t* piece_row = (int32_t*)(piece_edge + max_pieces);
  const size_t key32_bytes = ((size_t)nnz * 4 + 63) / 64 * 64;
  if ((rc = gm_graph_workspace(g, GM_WS_TC_KEYS, key32_bytes + 64, &p))) return rc;
  uint32_t* key32 = (uint32_t*)p;

  // gm_graph_last_stats afterwards: send_ms = the keys passes, spmv_ms = the plan and the count kernels (and the total's sum)
  gm_run_stats_t st;
  memset(&st, 0, sizeof(st));
  hipEvent_t ev[3];
  for (hipEvent_t& e : ev) GM_TRY_HIP(hipEventCreate(&e));
  GM_TRY_HIP(hipEventRecord(ev[0], s));
  GM_TRY_HIP(hipMemsetAsync(flags, 0, 64, s));
  uint32_t duplicates = 0;
  if (nnz > 0) {
    hipLaunchKernelGGL(k_tc_keys32, dim3(tc_grid(nnz, kTcBlock)), dim3(kTcBlock), 0, s, I, (const int32_t*)g->native_of_dev, key32, flags);
    GM_TRY_HIP(hipMemcpyAsync(&duplicates, &flags->duplicates, 4, hipMemcpyDeviceToHost, s));
    GM_TRY_HIP(hipStreamSynchronize(s));
  }
  if (!duplicates) {
    GM_TRY_HIP(hipEventRecord(ev[1], s));
    if ((rc = tc_count<uint32_t>(g, key32, cls, piece_row, piece_edge, flags, d_triangles, s))) return rc;
  } else {
    // the slot grows once per graph; a slot that moved has lost the 32-bit keys (the stream is idle: the flag has just been read)
    if ((rc = gm_graph_workspace(g, GM_WS_TC_KEYS, key32_bytes + (size_t)nnz * 8 + 128, &p))) return rc;
    if (p != (void*)key32) {
      key32 = (uint32_t*)p;
      hipLaunchKernelGGL(k_tc_keys32, dim3(tc_grid(nnz, kTcBlock)), dim3(kTcBlock), 0, s, I, (const int32_t*)g->native_of_dev, key32, flags);
    }
    uint64_t* key64 = (uint64_t*)((char*)p + key32_bytes);
    hipLaunchKernelGGL(k_tc_keys64, dim3(tc_grid(nnz, kTcBlock)), dim3(kTcBlock), 0, s, I, (const uint32_t*)key32, key64);
    GM_TRY_HIP(hipEventRecord(ev[1], s));
    if ((rc = tc_count<uint64_t>(g, key64, cls, piece_row, piece_edge, flags, d_triangles, s))) return rc;
  }
  if (h_total) {
    const unsigned grid = n > 0 ? (tc_grid(n, kTcBlock) < 1024u ? tc_grid(n, kTcBlock) : 1024u) : 0u;
    if (grid) hipLaunchKernelGGL(k_tc_total, dim3(grid), dim3(kTcBlock), 0, s, (const int64_t*)d_triangles, n, flags);
    unsigned long long total = 0;
    GM_TRY_HIP(hipMemcpyAsync(&total, &flags->total, 8, hipMemcpyDeviceToHost, s));
    GM_TRY_HIP(hipStreamSynchronize(s));
    *h_total = (uint64_t)total;
  }
  GM_TRY_HIP(hipEventRecord(ev[2], s));
  if (h_total) {  // (without h_total the call does not wait for the stream, and the times stay 0)
    GM_TRY_HIP(hipEventSynchronize(ev[2]));
    GM_TRY_HIP(hipEventElapsedTime(&st.send_ms, ev[0], ev[1]));
    GM_TRY_HIP(hipEventElapsedTime(&st.spmv_ms, ev[1], ev[2]));
    st.total_ms = st.send_ms + st.spmv_ms;
  }
  for (hipEvent_t& e : ev) (void)hipEventDestroy(e);
  st.iterations = 1;
  g->stats = st;
  return GM_OK;
}

}  // namespace gm

extern "C" int gm_run_triangle_count(gm_graph_t* g, int64_t* d_triangles, uint64_t* h_total, gm_stream_t stream) {
  // argument errors first: nothing on the GPU is touched
  if (!g || !d_triangles) { gm::set_error("gm_run_triangle_count: null graph or output array"); return GM_ERR_INVALID; }
  const gm_graph_desc_t& d = g->desc;
  if (!g->out.present || !g->in.present) { gm::set_error("gm_run_triangle_count: needs a graph built with both directions"); return GM_ERR_UNSUPPORTED; }
  if (d.row_lo != 0 || d.row_hi != d.ndevice || d.nshards > 1 || g->xfn != nullptr) {
    gm::set_error("gm_run_triangle_count: whole graphs only (no shards, no row ranges)");
    return GM_ERR_UNSUPPORTED;
  }
  return gm::run_triangle_count(g, d_triangles, h_total, (hipStream_t)stream);
}
