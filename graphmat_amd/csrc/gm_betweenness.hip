// gm_betweenness.hip -- betweenness centrality after Brandes (2001): per source a level-synchronous forward pass that counts
// shortest paths, then a backward pass over the levels that accumulates dependencies.  fp64.
//
// Unweighted, DIRECTED, unnormalised, endpoints not counted, on the simple directed graph under the edge list: duplicate edges
// count once, self-loops and edge values are ignored.  For the sources S:  bc[v] = sum over s in S of delta_s(v), delta_s(s) = 0,
//   sigma_s(w) = the number of shortest s -> w paths,
//   delta_s(v) = sum over v -> w with depth(w) = depth(v) + 1 of  sigma(v) / sigma(w) * (1 + delta_s(w))   (divide, then multiply).
// Only the GM_DIR_IN adjacency is read: its row v (rows = sources) holds v's out-neighbours, and both phases walk out-rows.  A row
// ascends in native ids (scc_bound of gm_scc.hip relies on it), so equal entries are neighbours: an entry equal to its predecessor
// in the row is a duplicate, an entry equal to the row's own id is a loop.  Both are checked per entry (bc_simple); no second
// edge array is built.
//
// Once per call:
//   k_bc_sources      src_dev[i] = the device id of the i-th source (vertex id -> native id -> device id; all vertices: i + 1)
//   k_bc_zero         bc[v] = 0 for every device slot
// Per source, one after the other on the stream:
//   k_bc_start        depth[v] = -1, sigma[v] = 0, delta[v] = 0; the source gets depth 0, sigma 1 and is order[0]; listed = 1, nlong = 0
//   (a) forward, level d = 0, 1, ...: the lists of all levels lie one after another in order[] (n entries: a vertex is listed once);
//       the host keeps the level offsets.  flags->listed counts all entries so far, flags->nlong all long rows so far.
//   k_bc_forward      a group of kBcLanes lanes per vertex u of level d walks u's out-row.  Per simple entry w: a look at depth[w];
//                     if it shows -1, atomicCAS(&depth[w], -1, d + 1); the lane whose CAS wins appends w to order[] (one atomic add
//                     per wave: ballot + popcount, scc_append); every lane that finds depth[w] == d + 1, by its look or by what its
//                     CAS returned, adds sigma[u] into sigma[w] with the hardware fp64 atomic (no compare-and-swap loop).
//                     A row of more than kBcLongRow entries is appended to long_list[] and handed to
//   k_bc_forward_long a long vertex per blockIdx.x, kBcLongBlocks workgroups striding over its row: the same step
//   (b) backward, level d = deepest - 1 down to 1 (the deepest level has no deeper neighbour: its delta stays 0; level 0 holds only
//       the source, whose delta is discarded).  A pull without float atomics: v of level d owns delta[v] and bc[v].
//   k_bc_backward     a group of kBcLanes lanes per v of level d: lane l sums the terms of the entries l, l + kBcLanes, ... of v's
//                     row in row order, then the lanes' sums are added in a fixed xor tree; delta[v] = the sum, bc[v] += the sum.
//                     Long rows are skipped here and summed by
//   k_bc_backward_long a workgroup per long vertex of level d (its part of long_list[]): thread t sums the entries t, t + 256, ...,
//                     then a fixed tree through LDS
// At the end depth[] and sigma[] of the last source are copied to the caller's arrays, if given.
//
// Bounds: a vertex enters order[] when a CAS on its depth wins, which happens once per source: at most n entries, and at most
// (rows longer than kBcLongRow) entries of long_list[]; both appends check their capacity all the same.  The levels of a source
// are at most n.  Every loop in a kernel runs over a row's or a list's length.  No kernel waits for another wave or workgroup,
// none is persistent or cooperative, nothing is retried (the fp64 add is one instruction).
// Known limit: a source costs about two launches per level and a 32-byte read per forward level, so deep graphs are slow; the
// sources run one after another (batching them is not built).
//
// Memory model.  Inside one launch a plain load may return an older value than another workgroup has written (a CU's L1, another
// XCD's L2); atomics are coherent.  depth[w] changes once per source, from -1 to its level, by a CAS: an older look can only show
// -1, and the CAS then returns the truth, so which lanes add and who appends is decided by values atomics returned or by a value
// that can no longer change.  sigma[u] of a level-d vertex was completed in the launches of level d - 1 and is read in a later
// launch; sigma[w] is only added to (atomics) during level d and read from the next launch on.  The backward pass of level d
// reads depth[], sigma[] (final since the forward phase) and delta[] of level d + 1 (written by the launch before) and writes
// only what its own vertex owns.  List lengths are read across kernel boundaries only (by the host).
// Determinism: while every sigma < 2^53 the forward sums are exact integers whatever their order; the backward sums have a fixed
// lane mapping and a fixed order, and bc[v] is added to source by source: two calls on one graph build return the same bytes.
// Measurements and the choices taken from them: profiles/betweenness.md.
#include <limits.h>
#include <string.h>

#include <vector>

#include "gm_internal.hpp"

namespace gm {

constexpr int kBcBlock = 256;       // (not measured: the block size of gm_scc.hip and gm_kcore.hip)
constexpr int kBcLanes = 16;        // lanes per listed vertex in k_bc_forward and k_bc_backward (measured: 4 / 8 / 16 / 32, profiles/betweenness.md (b))
constexpr int kBcLongRow = 256;     // rows of more entries go to the long kernels (measured: 256 / 512 / 1024 / never, profiles/betweenness.md (b))
constexpr int kBcLongBlocks = 32;   // workgroups per row of k_bc_forward_long (kSccLongBlocks)
static_assert(64 % kBcLanes == 0 && (kBcBlock & (kBcBlock - 1)) == 0, "whole groups per wave; the tree of k_bc_backward_long halves the block");

struct BcFlags {       // workspace slot GM_WS_BC_FLAG; the host reads all of it after every forward pass
  uint32_t listed;     // entries of order[] so far (this source)
  uint32_t nlong;      // entries of long_list[] so far (this source)
  uint32_t unused_[6];
};

struct BcRows { const int64_t* rowptr; const int32_t* colidx; };
struct BcWalk {        // what a forward step needs
  int32_t* depth;
  double* sigma;
  int32_t* order;
  uint32_t cap;        // entries of order[]
  BcFlags* flags;
};

__device__ __forceinline__ unsigned long long bc_below(int lane) { return (1ull << lane) - 1ull; }  // the lanes before `lane`

// order[old length ...] <- w of the lanes with `hit`: one atomic add per wave; every lane of the wave calls it (scc_append)
__device__ __forceinline__ void bc_append(bool hit, int w, int32_t* __restrict__ list, uint32_t* len, uint32_t cap) {
  const unsigned long long m = __ballot(hit);
  if (m == 0) return;
  const int lane = threadIdx.x & 63, leader = __builtin_ctzll(m);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(len, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, leader);
  const uint32_t at = base + (uint32_t)__popcll(m & bc_below(lane));
  if (hit && at < cap) list[at] = w;
}

// entry p of row u (which starts at `at`) is an edge of the simple graph: no loop, and not the repetition of the entry before it
__device__ __forceinline__ bool bc_simple(const int32_t* __restrict__ colidx, int64_t at, int64_t p, int w, int u) {
  return w != u && (p == at || colidx[p - 1] != w);
}

// the forward step for entry p of u's row; every lane of the wave calls it
__device__ __forceinline__ void bc_visit(bool valid, const int32_t* __restrict__ colidx, int64_t at, int64_t p, int u, double su, int d, const BcWalk& W) {
  bool won = false;
  int w = 0;
  if (valid) {
    w = colidx[p];
    if (bc_simple(colidx, at, p, w, u)) {
      int dw = W.depth[w];  // (the look: an older value can only be -1, see the head of this file)
      if (dw == -1) {
        dw = atomicCAS(&W.depth[w], -1, d + 1);
        if (dw == -1) { won = true; dw = d + 1; }
      }
      if (dw == d + 1) unsafeAtomicAdd(&W.sigma[w], su);  // global_atomic_add_f64 (the workspace is hipMalloc'ed memory)
    }
  }
  bc_append(won, w, W.order, &W.flags->listed, W.cap);
}

// ---------------- once per call ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBcBlock)
k_bc_sources(const int32_t* __restrict__ src_vertex, int nsources, const int32_t* __restrict__ dev_of_native, int nparts, int nvertices,
             int32_t* __restrict__ src_dev) {
  const int i = blockIdx.x * kBcBlock + threadIdx.x;
  if (i >= nsources) return;
  const int native = to_native0(src_vertex ? src_vertex[i] : i + 1, nparts, nvertices);
  src_dev[i] = dev_of_native ? dev_of_native[native] : native;
}

__global__ void __launch_bounds__(kBcBlock)
k_bc_zero(double* __restrict__ bc, int n) {
  const int v = blockIdx.x * kBcBlock + threadIdx.x;
  if (v < n) bc[v] = 0.0;
}

// ---------------- per source ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBcBlock)
k_bc_start(int32_t* __restrict__ depth, double* __restrict__ sigma, double* __restrict__ delta, int n, const int32_t* __restrict__ src_dev, int i,
           int32_t* __restrict__ order, BcFlags* flags) {
  const int v = blockIdx.x * kBcBlock + threadIdx.x;
  if (v == 0) { flags->listed = 1u; flags->nlong = 0u; }
  if (v >= n) return;
  const bool is = v == src_dev[i];
  depth[v] = is ? 0 : -1;
  sigma[v] = is ? 1.0 : 0.0;
  delta[v] = 0.0;
  if (is) order[0] = v;
}

__global__ void __launch_bounds__(kBcBlock)
k_bc_forward(uint32_t first, uint32_t len, int d, BcRows A, BcWalk W, int32_t* __restrict__ long_list, uint32_t long_cap) {
  const uint64_t t = (uint64_t)blockIdx.x * kBcBlock + threadIdx.x, grp = t / kBcLanes;
  const int gl = (int)(t % kBcLanes);
  int u = -1;
  int64_t at = 0, end = 0;
  double su = 0.0;
  if (grp < len) {
    u = W.order[first + grp];
    su = W.sigma[u];
    at = A.rowptr[u];
    end = A.rowptr[u + 1];
    if (end - at > kBcLongRow) {
      if (gl == 0) {  // (once per long row and source)
        const uint32_t i = atomicAdd(&W.flags->nlong, 1u);
        if (i < long_cap) long_list[i] = u;
      }
      end = at;
    }
  }
  int turns = (int)((end - at + kBcLanes - 1) / kBcLanes);  // <= kBcLongRow / kBcLanes; the wave's largest, so that every lane stays in the loop
#pragma unroll
  for (int o = 32; o >= kBcLanes; o >>= 1) { const int y = __shfl_xor(turns, o); turns = y > turns ? y : turns; }
  int64_t p = at + gl;
  for (int i = 0; i < turns; i++, p += kBcLanes) bc_visit(p < end, A.colidx, at, p, u, su, d, W);
}

__global__ void __launch_bounds__(kBcBlock)
k_bc_forward_long(const int32_t* __restrict__ long_list, uint32_t lfirst, int d, BcRows A, BcWalk W) {
  const int u = long_list[lfirst + blockIdx.x];
  const double su = W.sigma[u];
  const int64_t at = A.rowptr[u], end = A.rowptr[u + 1];
  for (int64_t base = at + (int64_t)blockIdx.y * kBcBlock; base < end; base += (int64_t)kBcLongBlocks * kBcBlock) {
    const int64_t p = base + threadIdx.x;
    bc_visit(p < end, A.colidx, at, p, u, su, d, W);
  }
}

// the term of entry p of v's row (v of level d), 0 where the entry is no edge of the simple graph or does not lead one level down
__device__ __forceinline__ double bc_term(const int32_t* __restrict__ colidx, int64_t at, int64_t p, int v, double sv, int d,
                                          const int32_t* __restrict__ depth, const double* __restrict__ sigma, const double* __restrict__ delta) {
  const int w = colidx[p];
  if (!bc_simple(colidx, at, p, w, v) || depth[w] != d + 1) return 0.0;
  return sv / sigma[w] * (1.0 + delta[w]);  // (divide, then multiply: the build has -ffp-contract=off)
}

__global__ void __launch_bounds__(kBcBlock)
k_bc_backward(const int32_t* __restrict__ order, uint32_t first, uint32_t len, int d, BcRows A, const int32_t* __restrict__ depth,
              const double* __restrict__ sigma, double* __restrict__ delta, double* __restrict__ bc) {
  const uint64_t t = (uint64_t)blockIdx.x * kBcBlock + threadIdx.x, grp = t / kBcLanes;
  const int gl = (int)(t % kBcLanes);
  int v = -1;
  int64_t at = 0, end = 0;
  double sv = 0.0;
  if (grp < len) {
    v = order[first + grp];
    at = A.rowptr[v];
    end = A.rowptr[v + 1];
    if (end - at > kBcLongRow) { v = -1; end = at; }  // (k_bc_backward_long's)
    else sv = sigma[v];
  }
  double acc = 0.0;
  for (int64_t p = at + gl; p < end; p += kBcLanes) acc += bc_term(A.colidx, at, p, v, sv, d, depth, sigma, delta);
#pragma unroll
  for (int o = kBcLanes >> 1; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);  // (a + b == b + a: every lane of the group holds the same sum)
  if (v >= 0 && gl == 0) { delta[v] = acc; bc[v] += acc; }
}

__global__ void __launch_bounds__(kBcBlock)
k_bc_backward_long(const int32_t* __restrict__ long_list, uint32_t lfirst, int d, BcRows A, const int32_t* __restrict__ depth,
                   const double* __restrict__ sigma, double* __restrict__ delta, double* __restrict__ bc) {
  __shared__ double s_sum[kBcBlock];
  const int v = long_list[lfirst + blockIdx.x];
  const int64_t at = A.rowptr[v], end = A.rowptr[v + 1];
  const double sv = sigma[v];
  double acc = 0.0;
  for (int64_t p = at + threadIdx.x; p < end; p += kBcBlock) acc += bc_term(A.colidx, at, p, v, sv, d, depth, sigma, delta);
  s_sum[threadIdx.x] = acc;
  __syncthreads();
  for (int half = kBcBlock >> 1; half >= 1; half >>= 1) {
    if ((int)threadIdx.x < half) s_sum[threadIdx.x] += s_sum[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) { delta[v] = s_sum[0]; bc[v] += s_sum[0]; }
}

static inline unsigned bc_grid(int64_t n, int per_block = kBcBlock) { return n > 0 ? (unsigned)((n + per_block - 1) / per_block) : 1u; }  // (no empty grid)
static inline size_t bc_pad(size_t bytes) { return (bytes + 63) / 64 * 64; }

// ev[0..5]: created and destroyed by the caller, whatever this returns
static int betweenness(gm_graph_t* g, const int32_t* h_sources, int32_t nsources, double* d_bc, int32_t* d_last_depth, double* d_last_sigma,
                       hipStream_t s, hipEvent_t* ev) {
  const gm_csr_t& I = g->in.view;
  const int n = I.nrows;
  const BcRows A = {I.rowptr, I.colidx};
  const int total_sources = h_sources ? nsources : g->desc.nvertices;
  const size_t long_cap = (size_t)(I.nnz / kBcLongRow) + 2;  // rows of more than kBcLongRow entries: fewer than nnz / kBcLongRow
  int rc;
  void* p = nullptr;
  if ((rc = gm_graph_workspace(g, GM_WS_BC_FLAG, 64, &p))) return rc;
  BcFlags* flags = (BcFlags*)p;
  const size_t vbytes = bc_pad((size_t)n * 4), sbytes = bc_pad((size_t)total_sources * 4 + 4);
  if ((rc = gm_graph_workspace(g, GM_WS_BC_ORDER, vbytes + bc_pad(long_cap * 4) + 2 * sbytes + 64, &p))) return rc;
  char* at = (char*)p;
  int32_t* order = (int32_t*)at; at += vbytes;
  int32_t* long_list = (int32_t*)at; at += bc_pad(long_cap * 4);
  int32_t* src_vertex = (int32_t*)at; at += sbytes;
  int32_t* src_dev = (int32_t*)at;
  if ((rc = gm_graph_workspace(g, GM_WS_BC_STATE, 5 * vbytes + 64, &p))) return rc;
  at = (char*)p;
  double* sigma = (double*)at; at += 2 * vbytes;
  double* delta = (double*)at; at += 2 * vbytes;
  int32_t* depth = (int32_t*)at;
  const BcWalk W = {depth, sigma, order, (uint32_t)n, flags};

  // gm_graph_last_stats afterwards: send_ms = set-up, spmv_ms = the forward phases, apply_ms = the backward phases and the finish;
  // iterations = sources processed, spmv_launches = level passes, forward plus backward (the long rows' launches are not counted)
  gm_run_stats_t st;
  memset(&st, 0, sizeof(st));
  // the flags land in the graph's pinned block, as in gm_kcore.hip (measured there)
  BcFlags h_own;
  BcFlags& h = g->pinned_flag ? *(BcFlags*)g->pinned_flag : h_own;
  memset(&h, 0, sizeof(h));
  auto read_flags = [&]() -> int {
    GM_TRY_HIP(hipMemcpyAsync(&h, flags, sizeof(h), hipMemcpyDeviceToHost, s));
    GM_TRY_HIP(hipStreamSynchronize(s));
    return GM_OK;
  };
  // the time split: source i's forward phase runs from `begin` (the end of the set-up, or the end of source i - 1) to fwd_end[i & 1],
  // its backward phase from there to bwd_end[i & 1].  The forward phase is the only one the host waits in, so the events of
  // source i - 1 are read after the first wait of source i, before any of them is recorded again.
  hipEvent_t ev_start = ev[0], ev_setup = ev[1];
  hipEvent_t fwd_end[2] = {ev[2], ev[3]}, bwd_end[2] = {ev[4], ev[5]};
  auto account = [&](int i) -> int {  // source i, whose events have completed
    float ms = 0.f;
    GM_TRY_HIP(hipEventElapsedTime(&ms, i == 0 ? ev_setup : bwd_end[(i - 1) & 1], fwd_end[i & 1]));
    st.spmv_ms += ms;
    GM_TRY_HIP(hipEventElapsedTime(&ms, fwd_end[i & 1], bwd_end[i & 1]));
    st.apply_ms += ms;
    return GM_OK;
  };

  GM_TRY_HIP(hipEventRecord(ev_start, s));
  if (h_sources && nsources > 0) GM_TRY_HIP(hipMemcpyAsync(src_vertex, h_sources, (size_t)nsources * 4, hipMemcpyHostToDevice, s));
  if (total_sources > 0)
    hipLaunchKernelGGL(k_bc_sources, dim3(bc_grid(total_sources)), dim3(kBcBlock), 0, s, h_sources ? (const int32_t*)src_vertex : (const int32_t*)nullptr,
                       total_sources, (const int32_t*)g->dev_of_native, g->desc.nparts, g->desc.nvertices, src_dev);
  hipLaunchKernelGGL(k_bc_zero, dim3(bc_grid(n)), dim3(kBcBlock), 0, s, d_bc, n);
  if (total_sources == 0) {  // no source: depth -1 and sigma 0 everywhere
    if (d_last_depth) GM_TRY_HIP(hipMemsetAsync(d_last_depth, 0xff, (size_t)n * 4, s));
    if (d_last_sigma) GM_TRY_HIP(hipMemsetAsync(d_last_sigma, 0, (size_t)n * 8, s));
  }
  GM_TRY_HIP(hipEventRecord(ev_setup, s));

  std::vector<uint32_t> off, loff;  // level d of the current source is order[off[d] .. off[d + 1]), its long rows long_list[loff[d] .. loff[d + 1])
  for (int i = 0; i < total_sources; i++) {
    hipLaunchKernelGGL(k_bc_start, dim3(bc_grid(n)), dim3(kBcBlock), 0, s, depth, sigma, delta, n, (const int32_t*)src_dev, i, order, flags);
    off.assign({0u, 1u});
    loff.assign({0u});
    int levels = 0;  // levels with vertices: 0 .. levels - 1
    for (int d = 0; d <= n; d++) {  // a level with vertices gives each of them its depth: at most n levels, and the pass that lists nothing
      const uint32_t first = off[d], len = off[d + 1] - first;
      if (len == 0) break;
      levels = d + 1;
      hipLaunchKernelGGL(k_bc_forward, dim3(bc_grid((int64_t)len * kBcLanes)), dim3(kBcBlock), 0, s, first, len, d, A, W, long_list, (uint32_t)long_cap);
      if ((rc = read_flags())) return rc;
      st.spmv_launches++;
      if (d == 0 && i > 0 && (rc = account(i - 1))) return rc;
      const uint32_t lnow = h.nlong < (uint32_t)long_cap ? h.nlong : (uint32_t)long_cap;
      loff.push_back(lnow);
      if (lnow > loff[d]) {
        hipLaunchKernelGGL(k_bc_forward_long, dim3(lnow - loff[d], kBcLongBlocks), dim3(kBcBlock), 0, s, (const int32_t*)long_list, loff[d], d, A, W);
        if ((rc = read_flags())) return rc;
      }
      off.push_back(h.listed < (uint32_t)n ? h.listed : (uint32_t)n);
    }
    GM_TRY_HIP(hipEventRecord(fwd_end[i & 1], s));
    for (int d = levels - 2; d >= 1; d--) {
      const uint32_t first = off[d], len = off[d + 1] - first;
      hipLaunchKernelGGL(k_bc_backward, dim3(bc_grid((int64_t)len * kBcLanes)), dim3(kBcBlock), 0, s, (const int32_t*)order, first, len, d, A, (const int32_t*)depth,
                         (const double*)sigma, delta, d_bc);
      if (loff[d + 1] > loff[d])
        hipLaunchKernelGGL(k_bc_backward_long, dim3(loff[d + 1] - loff[d]), dim3(kBcBlock), 0, s, (const int32_t*)long_list, loff[d], d, A, (const int32_t*)depth,
                           (const double*)sigma, delta, d_bc);
      st.spmv_launches++;
    }
    if (i == total_sources - 1) {
      if (d_last_depth) GM_TRY_HIP(hipMemcpyAsync(d_last_depth, depth, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
      if (d_last_sigma) GM_TRY_HIP(hipMemcpyAsync(d_last_sigma, sigma, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    }
    GM_TRY_HIP(hipEventRecord(bwd_end[i & 1], s));
    st.iterations = i + 1;
  }
  GM_TRY_HIP(hipStreamSynchronize(s));
  GM_TRY_HIP(hipGetLastError());
  if (total_sources > 0 && (rc = account(total_sources - 1))) return rc;
  GM_TRY_HIP(hipEventElapsedTime(&st.send_ms, ev_start, ev_setup));
  st.total_ms = st.send_ms + st.spmv_ms + st.apply_ms;
  g->stats = st;
  return GM_OK;
}

static int run_betweenness(gm_graph_t* g, const int32_t* h_sources, int32_t nsources, double* d_bc, int32_t* d_last_depth, double* d_last_sigma, hipStream_t s) {
  if (g->in.view.nrows <= 0) return GM_OK;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int rc = GM_OK;
  for (hipEvent_t& e : ev) {
    if (rc == GM_OK && hipEventCreate(&e) != hipSuccess) { set_error("gm_run_betweenness: hipEventCreate failed"); rc = GM_ERR_HIP; }
  }
  if (rc == GM_OK) rc = betweenness(g, h_sources, nsources, d_bc, d_last_depth, d_last_sigma, s, ev);
  for (hipEvent_t& e : ev) if (e) (void)hipEventDestroy(e);
  return rc;
}

}  // namespace gm

extern "C" int gm_run_betweenness(gm_graph_t* g, const int32_t* h_sources, int32_t nsources, double* d_bc, int32_t* d_last_depth, double* d_last_sigma,
                                  gm_stream_t stream) {
  // argument errors first: nothing on the GPU is touched
  if (!g || !d_bc) { gm::set_error("gm_run_betweenness: null graph or output array"); return GM_ERR_INVALID; }
  if (nsources < 0) { gm::set_error("gm_run_betweenness: nsources = %d is negative", nsources); return GM_ERR_INVALID; }
  if (!h_sources && nsources > 0) { gm::set_error("gm_run_betweenness: null source array with nsources = %d", nsources); return GM_ERR_INVALID; }
  for (int32_t i = 0; i < nsources; i++) {
    if (h_sources[i] < 1) { gm::set_error("gm_run_betweenness: source id %d outside 1..nv", h_sources[i]); return GM_ERR_INVALID; }
  }
  const gm_graph_desc_t& d = g->desc;
  if (d.row_lo != 0 || d.row_hi != d.ndevice || d.nshards > 1 || g->xfn != nullptr) {
    gm::set_error("gm_run_betweenness: whole graphs only (no shards, no row ranges)");
    return GM_ERR_UNSUPPORTED;
  }
  if (!g->in.present) {
    gm::set_error("gm_run_betweenness: needs the GM_DIR_IN adjacency (a graph built with GM_DIR_IN; its rows hold the out-neighbours)");
    return GM_ERR_UNSUPPORTED;
  }
  for (int32_t i = 0; i < nsources; i++) {
    if (h_sources[i] > d.nvertices) { gm::set_error("gm_run_betweenness: source id %d outside 1..%d", h_sources[i], d.nvertices); return GM_ERR_INVALID; }
  }
  return gm::run_betweenness(g, h_sources, nsources, d_bc, d_last_depth, d_last_sigma, (hipStream_t)stream);
}
