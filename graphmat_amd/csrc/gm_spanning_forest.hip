// gm_spanning_forest.hip -- minimum spanning forest by Boruvka rounds: pick, hook, jump; exact integers.
//
// The graph is the UNDIRECTED MULTIGRAPH under the edge list: directions do not matter, self-loops are ignored, parallel and
// antiparallel edges are separate candidates.  A weight is the 4-byte edge value read as signed int32 (a graph without values
// weighs every edge 1).  ONE adjacency is read (GM_DIR_OUT when the graph has it, else GM_DIR_IN): every input edge stands in it
// once, at CSR position e.  The order of the candidates is the order of
//     key(e) = (uint64(uint32(w) ^ 0x80000000) << 32) | e
// -- the weight with its sign bit flipped compares as the signed weight does, the position breaks ties --, a STRICT TOTAL order over
// the entries because no two share a position.  nnz < 2^32 - 1, so no key is ~0, the value of an empty best[] word.
//
// State over DEVICE ids (n = the adjacency's rows):
//   comp[v]     the root of v's tree (a root has comp[r] == r); between rounds every entry is a root
//   best[r]     uint64, per root: the smallest key among the entries that leave r's tree, or ~0
//   hook[v]     this round's parent of v: for a root its new parent or itself, for every other vertex comp[v]
//   edge_of[v]  the CSR position through which slot v was hooked, or none
//   k_msf_init        comp[v] = v, best[v] = ~0, edge_of[v] = none, the flags block cleared
//   k_cc_edge_rows    once per call (gm_edge_rows.hpp): row_of_edge[e], so that every edge kernel has lane = edge
//   k_msf_pick        lane = entry e = (u, v): cu = comp[u], cv = comp[v]; where they differ, the 64-bit atomic minimum of key(e) into
//                     best[cu] and best[cv] (after a look, and combined within the wave: below); one store per wave that saw a
//                     difference marks the round as one that found work
//   k_msf_hook        lane = vertex r, a root with best[r] set: e = low32(best[r]), other = the root of e's endpoint outside r's tree.
//                     If best[other] == best[r] and r < other, r stays a root; otherwise hook[r] = other, edge_of[r] = e
//   k_msf_jump        lane = vertex: follows hook[] from hook[v] for at most `steps` entries, writes where it got to into comp[v] and
//                     hook[v], resets best[] of a root, and marks the pass as unfinished where the walk ended below a root
//   k_msf_emit        lane = slot: where edge_of is set, (min, max) of the entry's two VERTEX ids and its weight, else (0, 0, 0);
//                     the number of edges and the int64 total with one atomic each per wave
// The host repeats pick + hook + jump, reads the flags block once (into pinned memory), repeats the jump pass while it was
// unfinished, and stops after the first pick pass that marked nothing.
//
// No cycles.  Every tree with an entry that leaves it picks the smallest such entry under the strict total order above.  Suppose
// the choices closed a cycle of trees T1 -> T2 -> ... -> Tk -> T1 (k >= 2), Ti hooking through entry ei.  ei leaves Ti and enters
// Ti+1, so it leaves Ti+1 as well, and Ti+1 picked its smallest: key(ei+1) <= key(ei) for every i, around the cycle, hence all
// keys are equal, hence -- the order is strict -- all ei are ONE entry.  One entry joins two trees, so k = 2: the only possible
// cycle is the mutual pick of the same entry, which k_msf_hook sees as best[other] == best[r] and breaks by keeping the smaller
// device id a root.  (Two different entries between the same two trees cannot be picked mutually: each tree sees both.)  So
// hook[] is a forest, every walk along it ends in a root after at most n - 1 entries, and a slot that is hooked is never a root
// again: every slot receives at most one edge in the whole call, which is the output placement -- no compaction, no atomics, and
// a second call writes the same bytes.  The result is the minimum spanning forest because each hooked entry is the lightest one
// across a cut (the cut property, with ties ordered by position).
//
// Rounds.  A round whose pick pass finds work merges every tree that has a leaving entry with at least one other, so the number of
// such trees at least halves: at most floor(log2(nvertices)) passes find work (unused device slots have no entries).  That number,
// plus the last, empty pass, bounds the host loop.  Jump passes: with steps >= 1 a pass at least halves every vertex's distance
// to its root, so at most ceil(log2(n)) + 1 of them per round; the loop in the kernel runs `steps` times at the most.
//
// Memory model.  Inside one launch a plain load may return an older value than another workgroup has written (a CU's L1, another
// XCD's L2); atomics are coherent.  Nothing here needs more.  k_msf_pick reads comp[] and changes best[] by atomic minimum only,
// whose effect does not depend on what its thread read; the look before it is a load past the CU's L1, and a word only ever
// decreases within the launch, so one seen at or below the lane's key -- however old the value seen -- needs no atomic.  k_msf_hook
// reads comp[] and best[] and writes hook[] and edge_of[]: it reads no array that the same launch writes -- an endpoint may itself
// be a root that is being hooked, which is why the choice goes into hook[] and is applied by the next kernel.  k_msf_jump reads
// and writes hook[]: an older hook[x] is an older ancestor of x in the same tree, a root's entry never changes in the launch, and
// an entry that is no root is only ever replaced by one of its proper ancestors, so hook[x] == x can only be read of a real root.
// Whether a round found work and whether a jump pass finished is decided across kernel boundaries only (the host reads the
// flags).  No kernel waits for another wave or workgroup, nothing is retried.
//
// Atomics to one address are served one after the other, and from the second round on most entries that still join two trees
// address one word: the giant tree's.  So k_msf_pick looks first, and the lanes of a wave that share the first active lane's root
// hand that lane their smallest key first (a row's entries are neighbours in the wave, and the giant tree is most lanes' root).
// Measured on RMAT-22: 129 ms a call without the look, 7.1 ms with it, 4.3 ms with both (profiles/spanning_forest.md).
// gm_set_option("msf_form", f) is the measurement knob for this; results do not depend on it.  Bit 0: no look before the atomic.
// Bit 1: no combining within the wave.  Bits 2-3: the jump pass walks kMsfSteps entries (0, the default), 1 entry (pointer
// doubling: 4) or n entries (one pass per round: 8).
#include <limits.h>
#include <string.h>

#include "gm_edge_rows.hpp"  // k_cc_edge_rows, kCcBlock, kCcPiece, cc_grid
#include "gm_internal.hpp"

namespace gm {

int g_msf_form = GM_MSF_FORM_DEFAULT;

constexpr int kMsfBlock = kCcBlock;
constexpr int kMsfSteps = 32;  // entries a thread follows in one jump pass (measured: 1 / 32 / n, profiles/spanning_forest.md)
constexpr unsigned long long kMsfNone = ~0ull;
constexpr uint32_t kMsfNoEdge = 0xFFFFFFFFu;

struct MsfFlags {        // workspace slot GM_WS_MSF_FLAG
  uint32_t found_work;   // the last pick pass (counted from 1) that saw an entry between two trees
  uint32_t unfinished;   // the last jump pass (counted from 1 over the whole call) that left a vertex below its root
  uint32_t nedges;
  uint32_t pad;
  unsigned long long total;  // the int64 sum of the weights, added modulo 2^64
};

__device__ __forceinline__ int msf_vertex1(const int32_t* __restrict__ native_of_dev, int dev, int nparts, int nvertices) {
  return to_vertex1(native_of_dev ? native_of_dev[dev] : dev, nparts, nvertices);
}

// the atomic minimum of `key` into a[root] for the lanes with `active` (a[] only ever decreases during the launch); every lane of
// the wave calls it.  COMBINE: the active lanes that share the first active lane's root give their minimum to that lane, which
// acts for them.  LOOK: a load past this CU's L1 first; the value may be an older one, which only costs an atomic that changes nothing.
template <bool LOOK, bool COMBINE>
__device__ __forceinline__ void msf_min_into(unsigned long long* a, bool active, int root, unsigned long long key) {
  if (COMBINE) {
    const unsigned long long m = __ballot(active);
    if (m == 0) return;
    const int first = __ffsll((long long)m) - 1;
    const bool same = active && root == __shfl(root, first);
    unsigned long long x = same ? key : kMsfNone;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const unsigned long long y = __shfl_xor(x, o); x = y < x ? y : x; }
    if (same) { active = (int)(threadIdx.x & 63) == first; key = x; }
  }
  if (!active) return;
  if (LOOK && __hip_atomic_load(&a[root], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;
  atomicMin(&a[root], key);
}

__global__ void __launch_bounds__(kMsfBlock)
k_msf_init(int32_t* __restrict__ comp, unsigned long long* __restrict__ best, uint32_t* __restrict__ edge_of, int n, MsfFlags* __restrict__ flags) {
  const int v = blockIdx.x * kMsfBlock + threadIdx.x;
  if (v == 0) { flags->found_work = 0u; flags->unfinished = 0u; flags->nedges = 0u; flags->pad = 0u; flags->total = 0ull; }
  if (v >= n) return;
  comp[v] = v;
  best[v] = kMsfNone;
  edge_of[v] = kMsfNoEdge;
}

template <bool LOOK, bool COMBINE>
__global__ void __launch_bounds__(kMsfBlock)
k_msf_pick(const int32_t* __restrict__ row_of_edge, const int32_t* __restrict__ colidx, const int32_t* __restrict__ vals, int64_t nnz,
           const int32_t* __restrict__ comp, unsigned long long* best, uint32_t round, MsfFlags* __restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * kMsfBlock + threadIdx.x;
  bool differ = false;
  int cu = 0, cv = 0;
  unsigned long long key = kMsfNone;
  if (e < nnz) {
    cu = comp[row_of_edge[e]];
    cv = comp[colidx[e]];
    differ = cu != cv;
    if (differ) {  // (from the second round on most entries lie inside one tree: their weights are not loaded)
      const uint32_t w = vals ? (uint32_t)vals[e] : 1u;
      key = ((unsigned long long)(w ^ 0x80000000u) << 32) | (unsigned long long)(uint32_t)e;
    }
  }
  msf_min_into<LOOK, COMBINE>(best, differ, cu, key);
  msf_min_into<LOOK, COMBINE>(best, differ, cv, key);
  if (__any(differ) && (threadIdx.x & 63) == 0) flags->found_work = round;  // (every wave stores the same value)
}

__global__ void __launch_bounds__(kMsfBlock)
k_msf_hook(const int32_t* __restrict__ row_of_edge, const int32_t* __restrict__ colidx, const int32_t* __restrict__ comp,
           const unsigned long long* __restrict__ best, int32_t* __restrict__ hook, uint32_t* __restrict__ edge_of, int n) {
  const int r = blockIdx.x * kMsfBlock + threadIdx.x;
  if (r >= n) return;
  const int c = comp[r];
  int parent = c;
  if (c == r) {
    const unsigned long long b = best[r];
    if (b != kMsfNone) {
      const uint32_t e = (uint32_t)b;  // (a position that k_msf_pick wrote: below nnz; one of its endpoints lies in r's tree)
      const int cu = comp[row_of_edge[e]], cv = comp[colidx[e]];
      const int other = cu == r ? cv : cu;
      if (!(best[other] == b && r < other)) {  // the mutual pick of one entry: the smaller id stays a root
        parent = other;
        edge_of[r] = e;
      }
    }
  }
  hook[r] = parent;
}

__global__ void __launch_bounds__(kMsfBlock)
k_msf_jump(int32_t* hook, int32_t* __restrict__ comp, unsigned long long* __restrict__ best, int n, int steps, uint32_t pass,
           MsfFlags* __restrict__ flags) {
  const int v = blockIdx.x * kMsfBlock + threadIdx.x;
  bool below = false;
  if (v < n) {
    int p = hook[v];
    int pp = hook[p];
    for (int i = 1; i < steps && pp != p; i++) {  // at most `steps` entries; hook[] is a forest, so fewer than n are ever needed
      p = pp;
      pp = hook[p];
    }
    below = pp != p;
    if (below) p = pp;
    hook[v] = p;
    comp[v] = p;
    if (p == v) best[v] = kMsfNone;  // a root: next round's minimum starts empty
  }
  if (__any(below) && (threadIdx.x & 63) == 0) flags->unfinished = pass;  // (every wave stores the same value)
}

__global__ void __launch_bounds__(kMsfBlock)
k_msf_emit(const uint32_t* __restrict__ edge_of, const int32_t* __restrict__ row_of_edge, const int32_t* __restrict__ colidx,
           const int32_t* __restrict__ vals, const int32_t* __restrict__ native_of_dev, int n, int nparts, int nvertices,
           int32_t* __restrict__ edges, MsfFlags* __restrict__ flags) {
  const int v = blockIdx.x * kMsfBlock + threadIdx.x;
  uint32_t e = kMsfNoEdge;
  if (v < n) {
    e = edge_of[v];
    int a = 0, b = 0, w = 0;
    if (e != kMsfNoEdge) {
      const int x = msf_vertex1(native_of_dev, row_of_edge[e], nparts, nvertices), y = msf_vertex1(native_of_dev, colidx[e], nparts, nvertices);
      a = x < y ? x : y;
      b = x < y ? y : x;
      w = vals ? vals[e] : 1;
    }
    edges[(int64_t)v * 3 + 0] = a;
    edges[(int64_t)v * 3 + 1] = b;
    edges[(int64_t)v * 3 + 2] = w;
  }
  const bool set = e != kMsfNoEdge;
  const unsigned count = (unsigned)__popcll(__ballot(set));
  if (count == 0) return;
  long long sum = set ? (long long)(vals ? vals[e] : 1) : 0ll;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&flags->nedges, count);
    atomicAdd(&flags->total, (unsigned long long)sum);
  }
}

static inline size_t msf_pad(size_t bytes) { return (bytes + 63) / 64 * 64; }
static inline int msf_floor_log2(int64_t x) { int l = 0; while (x > 1) { x >>= 1; l++; } return l; }

static void msf_launch_pick(int form, unsigned grid, hipStream_t s, const int32_t* row_of_edge, const int32_t* colidx, const int32_t* vals, int64_t nnz,
                            const int32_t* comp, unsigned long long* best, uint32_t round, MsfFlags* flags) {
  const dim3 g(grid), b(kMsfBlock);
  switch (form & 3) {
    case 0: hipLaunchKernelGGL((k_msf_pick<true, true>), g, b, 0, s, row_of_edge, colidx, vals, nnz, comp, best, round, flags); break;
    case 1: hipLaunchKernelGGL((k_msf_pick<false, true>), g, b, 0, s, row_of_edge, colidx, vals, nnz, comp, best, round, flags); break;
    case 2: hipLaunchKernelGGL((k_msf_pick<true, false>), g, b, 0, s, row_of_edge, colidx, vals, nnz, comp, best, round, flags); break;
    default: hipLaunchKernelGGL((k_msf_pick<false, false>), g, b, 0, s, row_of_edge, colidx, vals, nnz, comp, best, round, flags); break;
  }
}

static int run_spanning_forest(gm_graph_t* g, int32_t* d_edges, int32_t* h_nedges, int64_t* h_total, hipStream_t s) {
  const gm_csr_t& A = g->out.present ? g->out.view : g->in.view;  // either adjacency holds every edge once
  const int n = A.nrows;
  const int64_t nnz = A.nnz;
  const int32_t* vals = A.val_bytes == 4 ? (const int32_t*)A.vals : nullptr;  // null: every edge weighs 1
  const int form = g_msf_form;
  if (n <= 0) { if (h_nedges) *h_nedges = 0; if (h_total) *h_total = 0; return GM_OK; }
  int rc;
  void* p = nullptr;
  if ((rc = gm_graph_workspace(g, GM_WS_MSF_FLAG, 64, &p))) return rc;
  MsfFlags* flags = (MsfFlags*)p;
  const size_t vbytes = msf_pad((size_t)n * 4);
  if ((rc = gm_graph_workspace(g, GM_WS_MSF_STATE, msf_pad((size_t)n * 8) + 3 * vbytes + 64, &p))) return rc;
  unsigned long long* best = (unsigned long long*)p;
  int32_t* comp = (int32_t*)((char*)p + msf_pad((size_t)n * 8));
  int32_t* hook = (int32_t*)((char*)comp + vbytes);
  uint32_t* edge_of = (uint32_t*)((char*)hook + vbytes);
  if ((rc = gm_graph_workspace(g, GM_WS_MSF_EDGE_ROWS, (size_t)nnz * 4 + 64, &p))) return rc;
  int32_t* row_of_edge = (int32_t*)p;
  const int steps = (form & 12) == 4 ? 1 : (form & 12) == 8 ? n : kMsfSteps;

  // gm_graph_last_stats afterwards: send_ms = init + edge rows, spmv_ms = the rounds, apply_ms = emit; iterations = pick passes,
  // spmv_launches = jump passes
  gm_run_stats_t st;
  memset(&st, 0, sizeof(st));
  hipEvent_t ev[4];
  for (hipEvent_t& e : ev) GM_TRY_HIP(hipEventCreate(&e));
  GM_TRY_HIP(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(k_msf_init, dim3(cc_grid(n)), dim3(kMsfBlock), 0, s, comp, best, edge_of, n, flags);
  if (nnz > 0) hipLaunchKernelGGL(k_cc_edge_rows, dim3(cc_grid(nnz, kCcPiece)), dim3(kCcBlock), 0, s, A, row_of_edge);
  GM_TRY_HIP(hipEventRecord(ev[1], s));
  // the flags land in the graph's pinned block (a run's own; runs on one graph follow each other), as in gm_kcore.hip
  MsfFlags h_own;
  MsfFlags& h = g->pinned_flag ? *(MsfFlags*)g->pinned_flag : h_own;
  memset(&h, 0, sizeof(h));
  bool done = nnz == 0;
  if (nnz > 0) {
    const int max_rounds = msf_floor_log2(g->desc.nvertices) + 1;  // passes that find work (see the head of this file) and the empty one
    const int max_jumps = msf_floor_log2(n) + 2;                   // jump passes of one round: ceil(log2(n)) + 1 at the most
    uint32_t pass = 0;
    for (int round = 1; round <= max_rounds && !done; round++) {
      msf_launch_pick(form, cc_grid(nnz), s, row_of_edge, A.colidx, vals, nnz, comp, best, (uint32_t)round, flags);
      hipLaunchKernelGGL(k_msf_hook, dim3(cc_grid(n)), dim3(kMsfBlock), 0, s, (const int32_t*)row_of_edge, A.colidx, (const int32_t*)comp,
                         (const unsigned long long*)best, hook, edge_of, n);
      for (int j = 0; j < max_jumps; j++) {
        hipLaunchKernelGGL(k_msf_jump, dim3(cc_grid(n)), dim3(kMsfBlock), 0, s, hook, comp, best, n, steps, ++pass, flags);
        GM_TRY_HIP(hipMemcpyAsync(&h, flags, sizeof(h), hipMemcpyDeviceToHost, s));
        GM_TRY_HIP(hipStreamSynchronize(s));
        st.spmv_launches++;
        if (h.unfinished != pass) break;
      }
      st.iterations = round;
      if (h.unfinished == pass) { set_error("gm_run_spanning_forest: a jump did not reach the roots within its bound"); return GM_ERR_HIP; }
      done = h.found_work != (uint32_t)round;
    }
  }
  if (!done) { set_error("gm_run_spanning_forest: the rounds did not end within floor(log2(nvertices)) + 1 passes"); return GM_ERR_HIP; }
  GM_TRY_HIP(hipEventRecord(ev[2], s));
  hipLaunchKernelGGL(k_msf_emit, dim3(cc_grid(n)), dim3(kMsfBlock), 0, s, (const uint32_t*)edge_of, (const int32_t*)row_of_edge, A.colidx, vals,
                     g->native_of_dev, n, g->desc.nparts, g->desc.nvertices, d_edges, flags);
  GM_TRY_HIP(hipMemcpyAsync(&h, flags, sizeof(h), hipMemcpyDeviceToHost, s));
  GM_TRY_HIP(hipEventRecord(ev[3], s));
  GM_TRY_HIP(hipEventSynchronize(ev[3]));
  GM_TRY_HIP(hipGetLastError());
  if (h_nedges) *h_nedges = (int32_t)h.nedges;
  if (h_total) *h_total = (int64_t)h.total;
  GM_TRY_HIP(hipEventElapsedTime(&st.send_ms, ev[0], ev[1]));
  GM_TRY_HIP(hipEventElapsedTime(&st.spmv_ms, ev[1], ev[2]));
  GM_TRY_HIP(hipEventElapsedTime(&st.apply_ms, ev[2], ev[3]));
  st.total_ms = st.send_ms + st.spmv_ms + st.apply_ms;
  for (hipEvent_t& e : ev) (void)hipEventDestroy(e);
  g->stats = st;
  return GM_OK;
}

}  // namespace gm

extern "C" int gm_run_spanning_forest(gm_graph_t* g, int32_t* d_edges, int32_t* h_nedges, int64_t* h_total, gm_stream_t stream) {
  // argument errors first: nothing on the GPU is touched
  if (!g || !d_edges || !h_nedges || !h_total) { gm::set_error("gm_run_spanning_forest: null graph or output pointer"); return GM_ERR_INVALID; }
  const gm_graph_desc_t& d = g->desc;
  if (d.row_lo != 0 || d.row_hi != d.ndevice || d.nshards > 1 || g->xfn != nullptr) {
    gm::set_error("gm_run_spanning_forest: whole graphs only (no shards, no row ranges)");
    return GM_ERR_UNSUPPORTED;
  }
  if (!g->out.present && !g->in.present) { gm::set_error("gm_run_spanning_forest: the graph holds no adjacency"); return GM_ERR_UNSUPPORTED; }
  const gm_csr_t& A = g->out.present ? g->out.view : g->in.view;
  if (A.val_bytes != 0 && A.val_bytes != 4) {
    gm::set_error("gm_run_spanning_forest: edge values of %d bytes (a weight is a 4-byte signed integer)", (int)A.val_bytes);
    return GM_ERR_UNSUPPORTED;
  }
  if (A.nnz >= 0xFFFFFFFFll) { gm::set_error("gm_run_spanning_forest: %lld edges (the key holds a 32-bit position)", (long long)A.nnz); return GM_ERR_UNSUPPORTED; }
  return gm::run_spanning_forest(g, d_edges, h_nedges, h_total, (hipStream_t)stream);
}
