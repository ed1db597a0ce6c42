// gm_components.hip -- weakly connected components by rounds of min-hooking and pointer jumping, exact integers.
//
// labels[v] = the smallest 1-based VERTEX id of v's component (what apps/label_propagation.cpp prints); edge directions, duplicate
// edges and self-loops do not matter, so ONE adjacency is read: every edge stands in it once.
//
// parent[] is an int32 forest over DEVICE ids, kept in the caller's d_labels.  Invariant: parent[x] <= x, so a chain of parents
// strictly decreases, ends in a root (parent[r] == r) and every walk along it is bounded.
//   k_cc_init       parent[v] = v, vmin[v] = INT_MAX, the flags block cleared
//   k_cc_edge_rows  once per call: row_of_edge[e] for every CSR position, so that the hook kernel reads (row, column) of an edge
//                   coalesced with lane = edge and its balance does not depend on row lengths (a giant row is no special case);
//                   it lives in gm_edge_rows.hpp, which gm_spanning_forest.hip includes as well
//   k_cc_hook       lane = edge (u, v): ru = parent[u], rv = parent[v]; if they differ, atomicMin(&parent[max], min) and the round is
//                   marked as one that found work (one store per wave that saw a difference)
//   k_cc_jump       lane = vertex: parent[v] follows its chain to the root; a thread writes its own entry only
// The host repeats hook + jump until a hook pass marks nothing, reading one word per round.  Before a hook pass every parent[] is a
// root (the jump kernel ran), so a pass that sees a difference takes at least one root away for good (parent[max] < max from then
// on, and no entry ever becomes a root again): at most nrows passes find work, and the loop's bound is that number, not a cap.
//   k_cc_min        used slots: atomicMin(&vmin[parent[v]], vertex id of v); the roots among them are the components (one add per wave)
//   k_cc_labels     labels[v] = vmin[parent[v]] in place (a thread reads its own parent only); unused slots get 0
//
// Memory model.  Inside one launch a plain load may return an older value than another workgroup has written (a CU's L1, another
// XCD's L2); atomics are coherent.  Nothing here needs more: an older parent[x] is an older ancestor of x and still names x's
// component and still is >= the current one; every change to the forest in the hook pass is an atomicMin, whose effect does not depend
// on what its thread read; whether a round found work is decided across kernel boundaries only; in the jump kernel nobody hooks,
// so parent[x] == x can only be read of a real root.  No kernel waits for another wave or workgroup, nothing is retried, and every
// loop is bounded by the invariant above or by a length read from rowptr.
//
// Atomics to one address are served one after the other, and a skewed graph sends most of them to few addresses: the trees of its
// giant component (hook passes after the first), its root's vmin entry.  Measured on RMAT-22, a call took 161 ms that way, 132 ms
// of it in the rounds and 27 ms in k_cc_min.  So both kernels look first (cc_min_into): the words only ever decrease, hence one that
// is seen at or below the lane's value -- however old the value seen -- needs no atomic; the look is a load past the CU's L1, where a
// busy line would stay as it was for the whole launch.  That left the lanes in flight before the first small value lands; in k_cc_min the lanes
// of a wave that share the first lane's root hand it their minimum first (in the hook pass that measured no gain and is not done).
// Measurements: profiles/connected_components.md.
#include <limits.h>
#include <string.h>

#include "gm_edge_rows.hpp"  // k_cc_edge_rows, cc_row_of, kCcBlock, kCcPiece, cc_grid
#include "gm_internal.hpp"

namespace gm {

struct CcFlags {         // workspace slot GM_WS_CC_FLAG
  uint32_t found_work;   // the last hook pass (counted from 1) that saw an edge between two trees
  uint32_t ncomponents;
};

__device__ __forceinline__ bool cc_used(const int32_t* __restrict__ native_of_dev, int v) { return !native_of_dev || native_of_dev[v] >= 0; }

// atomicMin(&a[key], val) for the lanes with `active` (a[] only ever decreases during the launch); every lane of the wave calls it.
// combine: the active lanes that share the first active lane's key give their minimum to that lane, which acts for them.
template <bool COMBINE>
__device__ __forceinline__ void cc_min_into(int32_t* a, bool active, int key, int val) {
  if (COMBINE) {
    const unsigned long long m = __ballot(active);
    if (m == 0) return;
    const int first = __ffsll((long long)m) - 1;
    const bool same = active && key == __shfl(key, first);
    int x = same ? val : INT_MAX;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int y = __shfl_xor(x, o); x = y < x ? y : x; }
    if (same) { active = (int)(threadIdx.x & 63) == first; val = x; }
  }
  // the look: a load past this CU's L1; the value may still be an older one, which only costs an atomic that changes nothing
  if (active && __hip_atomic_load(&a[key], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > val) atomicMin(&a[key], val);
}

__global__ void __launch_bounds__(kCcBlock)
k_cc_init(int32_t* __restrict__ parent, int32_t* __restrict__ vmin, int n, CcFlags* __restrict__ flags) {
  const int v = blockIdx.x * kCcBlock + threadIdx.x;
  if (v == 0) { flags->found_work = 0u; flags->ncomponents = 0u; }
  if (v >= n) return;
  parent[v] = v;
  vmin[v] = INT_MAX;
}

__global__ void __launch_bounds__(kCcBlock)
k_cc_hook(const int32_t* __restrict__ row_of_edge, const int32_t* __restrict__ colidx, int64_t nnz, int32_t* parent, uint32_t round,
          CcFlags* __restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * kCcBlock + threadIdx.x;
  bool differ = false;
  int hi = 0, lo = 0;
  if (e < nnz) {
    const int ru = parent[row_of_edge[e]], rv = parent[colidx[e]];
    differ = ru != rv;
    hi = ru > rv ? ru : rv;
    lo = ru > rv ? rv : ru;
  }
  cc_min_into<false>(parent, differ, hi, lo);
  if (__any(differ) && (threadIdx.x & 63) == 0) flags->found_work = round;  // (every wave stores the same value)
}

__global__ void __launch_bounds__(kCcBlock)
k_cc_jump(int32_t* parent, int n) {
  const int v = blockIdx.x * kCcBlock + threadIdx.x;
  if (v >= n) return;
  int p = parent[v];
  for (;;) {  // p strictly decreases: at most p steps
    const int pp = parent[p];
    if (pp == p) break;
    p = pp;
    parent[v] = p;
  }
}

__global__ void __launch_bounds__(kCcBlock)
k_cc_min(const int32_t* __restrict__ parent, const int32_t* __restrict__ native_of_dev, int n, int nparts, int nvertices,
         int32_t* vmin, CcFlags* __restrict__ flags) {
  const int v = blockIdx.x * kCcBlock + threadIdx.x;
  const bool used = v < n && cc_used(native_of_dev, v);
  int r = 0, id = 0;
  if (used) {
    r = parent[v];
    id = to_vertex1(native_of_dev ? native_of_dev[v] : v, nparts, nvertices);
  }
  cc_min_into<true>(vmin, used, r, id);
  const unsigned roots = (unsigned)__popcll(__ballot(used && r == v));
  if (roots && (threadIdx.x & 63) == 0) atomicAdd(&flags->ncomponents, roots);
}

__global__ void __launch_bounds__(kCcBlock)
k_cc_labels(int32_t* __restrict__ labels, const int32_t* __restrict__ native_of_dev, int n, const int32_t* __restrict__ vmin) {
  const int v = blockIdx.x * kCcBlock + threadIdx.x;
  if (v >= n) return;
  labels[v] = cc_used(native_of_dev, v) ? vmin[labels[v]] : 0;
}

static int run_connected_components(gm_graph_t* g, int32_t* d_labels, int32_t* h_ncomponents, hipStream_t s) {
  const gm_csr_t& A = g->out.present ? g->out.view : g->in.view;  // either adjacency holds every edge once
  const int n = A.nrows;
  const int64_t nnz = A.nnz;
  int rc;
  void* p = nullptr;
  if ((rc = gm_graph_workspace(g, GM_WS_CC_FLAG, 64, &p))) return rc;
  CcFlags* flags = (CcFlags*)p;
  if ((rc = gm_graph_workspace(g, GM_WS_CC_MIN, (size_t)n * 4 + 64, &p))) return rc;
  int32_t* vmin = (int32_t*)p;
  if ((rc = gm_graph_workspace(g, GM_WS_CC_EDGE_ROWS, (size_t)nnz * 4 + 64, &p))) return rc;
  int32_t* row_of_edge = (int32_t*)p;
  int32_t* parent = d_labels;
  const int32_t* native_of_dev = g->native_of_dev;

  // gm_graph_last_stats afterwards: send_ms = init + edge rows, spmv_ms = the rounds, apply_ms = labels + count
  gm_run_stats_t st;
  memset(&st, 0, sizeof(st));
  hipEvent_t ev[4];
  for (hipEvent_t& e : ev) GM_TRY_HIP(hipEventCreate(&e));
  GM_TRY_HIP(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(k_cc_init, dim3(cc_grid(n > 0 ? n : 1)), dim3(kCcBlock), 0, s, parent, vmin, n, flags);
  if (nnz > 0) hipLaunchKernelGGL(k_cc_edge_rows, dim3(cc_grid(nnz, kCcPiece)), dim3(kCcBlock), 0, s, A, row_of_edge);
  GM_TRY_HIP(hipEventRecord(ev[1], s));
  if (nnz > 0) {
    for (int64_t round = 1; round <= (int64_t)n + 1; round++) {  // at most n passes find work (see the head of this file)
      hipLaunchKernelGGL(k_cc_hook, dim3(cc_grid(nnz)), dim3(kCcBlock), 0, s, (const int32_t*)row_of_edge, A.colidx, nnz, parent, (uint32_t)round, flags);
      hipLaunchKernelGGL(k_cc_jump, dim3(cc_grid(n)), dim3(kCcBlock), 0, s, parent, n);
      uint32_t found_work = 0;
      GM_TRY_HIP(hipMemcpyAsync(&found_work, &flags->found_work, 4, hipMemcpyDeviceToHost, s));
      GM_TRY_HIP(hipStreamSynchronize(s));
      st.iterations = (int32_t)round;
      if (found_work != (uint32_t)round) break;
    }
  }
  GM_TRY_HIP(hipEventRecord(ev[2], s));
  if (n > 0) {
    hipLaunchKernelGGL(k_cc_min, dim3(cc_grid(n)), dim3(kCcBlock), 0, s, (const int32_t*)parent, native_of_dev, n, g->desc.nparts, g->desc.nvertices, vmin,
                       flags);
    hipLaunchKernelGGL(k_cc_labels, dim3(cc_grid(n)), dim3(kCcBlock), 0, s, d_labels, native_of_dev, n, (const int32_t*)vmin);
  }
  uint32_t ncomponents = 0;
  GM_TRY_HIP(hipMemcpyAsync(&ncomponents, &flags->ncomponents, 4, hipMemcpyDeviceToHost, s));
  GM_TRY_HIP(hipEventRecord(ev[3], s));
  GM_TRY_HIP(hipEventSynchronize(ev[3]));
  GM_TRY_HIP(hipGetLastError());
  if (h_ncomponents) *h_ncomponents = (int32_t)ncomponents;
  GM_TRY_HIP(hipEventElapsedTime(&st.send_ms, ev[0], ev[1]));
  GM_TRY_HIP(hipEventElapsedTime(&st.spmv_ms, ev[1], ev[2]));
  GM_TRY_HIP(hipEventElapsedTime(&st.apply_ms, ev[2], ev[3]));
  st.total_ms = st.send_ms + st.spmv_ms + st.apply_ms;
  for (hipEvent_t& e : ev) (void)hipEventDestroy(e);
  g->stats = st;
  return GM_OK;
}

}  // namespace gm

extern "C" int gm_run_connected_components(gm_graph_t* g, int32_t* d_labels, int32_t* h_ncomponents, gm_stream_t stream) {
  // argument errors first: nothing on the GPU is touched
  if (!g || !d_labels) { gm::set_error("gm_run_connected_components: null graph or output array"); return GM_ERR_INVALID; }
  const gm_graph_desc_t& d = g->desc;
  if (d.row_lo != 0 || d.row_hi != d.ndevice || d.nshards > 1 || g->xfn != nullptr) {
    gm::set_error("gm_run_connected_components: whole graphs only (no shards, no row ranges)");
    return GM_ERR_UNSUPPORTED;
  }
  if (!g->out.present && !g->in.present) { gm::set_error("gm_run_connected_components: the graph holds no adjacency"); return GM_ERR_UNSUPPORTED; }
  return gm::run_connected_components(g, d_labels, h_ncomponents, (hipStream_t)stream);
}
