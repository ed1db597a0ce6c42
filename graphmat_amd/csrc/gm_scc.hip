// gm_scc.hip -- strongly connected components: trim to a fixpoint, then rounds of forward min-colouring and backward marking,
// exact integers.
//
// labels[v] = the smallest 1-based VERTEX id of v's strongly connected component.  Edge directions matter; duplicate edges and
// self-loops do not; a vertex without edges, or with a self-loop only, is its own component.  BOTH adjacencies are walked: row v of
// GM_DIR_OUT (rows = destinations) holds v's in-neighbours, row v of GM_DIR_IN (rows = sources) its out-neighbours.  Colours are
// vertex ids, not device ids: the rounds do not depend on the layout, and a root's colour already is the label.
//
// state[v]: dead (trimmed, removed or an unused slot), alive, listed (claimed for a trim pass), marked (in a root's SCC this round).
//   k_scc_init        vid[v] = the vertex id of device slot v, state[v] = alive for used slots, labels[v] = 0
//   k_scc_degrees     indeg[v] / outdeg[v] = the non-loop entries of row v of OUT / IN.  A row ascends in native ids, so its loops
//                     are the run between two binary searches for its own id; duplicates stay as entries
//   k_scc_edge_rows   row_of_edge[e] of the OUT adjacency, so that the edge passes run with lane = edge (k_cc_edge_rows)
// (a) Trim: a vertex without alive in-neighbours or without alive out-neighbours is a component of its own.
//   k_scc_first_list  lists the alive vertices with indeg == 0 or outdeg == 0 (one atomic add per wave: ballot + popcount)
//   k_scc_pass        a group of kSccLanes lanes per listed vertex v: labels[v] = vid[v], state[v] = dead; for each out-neighbour
//                     w != v: atomicSub(&indeg[w], 1); for each in-neighbour u != v: atomicSub(&outdeg[u], 1).  The thread whose
//                     atomic returns 1 claims the neighbour (atomicCAS on state[], alive -> listed) and appends it to the next
//                     list.  The claim is needed: a vertex can reach zero on both counters in one pass, or on one while it is
//                     listed for the other.  A row of more than kSccLongRow entries is handed to
//   k_scc_long        a (vertex, adjacency) pair per blockIdx.x, kSccLongBlocks workgroups striding over the row: the same step
// (b) A round, while alive vertices remain:
//   k_scc_compact     before the first round: both ends of every edge with two alive ends, in any order; the edge passes read these
//   k_scc_colour      colour[v] = vid[v] for alive v
//   k_scc_forward     lane = edge u -> w, both ends alive: atomicMin(&colour[w], colour[u]) after a look (cc_min_into); a wave in
//                     which an atomic lowered a word stores the pass's number.  Repeated until a pass lowers nothing
//   k_scc_roots       alive v with colour[v] == vid[v] are the roots: marked, counted (one add per wave)
//   k_scc_backward    lane = edge u -> w: w marked, u alive and unmarked, colour[u] == colour[w]: u is marked.  Until nothing is marked
//   k_scc_gather      lists the marked vertices; k_scc_pass runs over that list with labels[v] = colour[v] (the removal pass: the
//                     listed vertices are marked, not alive, so nobody claims them).  What it brings to zero is the first list
//                     of the next trim
// ncomponents = trimmed vertices (the host adds up the trim lists' lengths, each of which was added once per wave) + roots (added
// once per wave).
//
// Why it is right: colour[r] == vid[r] at the forward fixpoint means r has the smallest id among all its alive ancestors.  Its
// SCC lies inside that set, so the colour is the SCC's smallest id, and the vertices that reach r backwards along edges of one
// colour are exactly its SCC among the alive vertices.
// Bounds: every vertex is listed at most once in the whole call (a claim happens once, a marked vertex dies in its round), so the
// trim and removal passes are at most n, and each entry of a vertex's two rows is decremented at most once: no counter passes
// below zero.  A round removes at least the SCC of the smallest alive id: at most n rounds.  A forward or backward pass that
// changes something lowers a colour or sets a mark: at most n + 1 passes a phase.  The loops in kernels run over a row's or a
// list's length.  No kernel waits for another wave or workgroup, none is persistent or cooperative, nothing is retried.
// Known limit: the passes grow with the longest chain that trimming peels and with the longest shortest path inside an SCC (a
// directed cycle of L vertices takes about L forward and L backward passes, each a launch and a 32-byte read).
//
// Memory model.  Inside one launch a plain load may return an older value than another workgroup has written (a CU's L1, another
// XCD's L2); atomics are coherent.  Nothing here needs more.  Colours only decrease and marks only get set, so an older value only
// delays an update to the next pass; a pass that wrote nothing read only current values (everything it read was written before
// the launch), so "no change" proves the fixpoint.  Whether a pass changed something is decided by the value atomicMin returns
// (forward) or by the thread's own store (backward).  In the trim, who appends a vertex is decided by the values the atomics
// return (the counter's 1, then the claim's "alive"), never by a plain read.  The look at state[x] before a decrement is a plain
// load: a vertex never becomes alive again, so "not alive" is true whenever it is read, and such a vertex's counters are never read
// again; an older "alive" costs one atomic whose claim fails.  List lengths, flags, the state[] transitions between phases and
// the frozen colours of the backward phase are read across kernel boundaries only (the lengths by the host).
// Measurements and the choices taken from them: profiles/scc.md.
#include <limits.h>
#include <string.h>

#include "gm_internal.hpp"

namespace gm {

constexpr int kSccBlock = 256;       // (not measured: the block size of gm_components.hip and gm_kcore.hip)
constexpr int kSccPiece = 4096;      // edges per workgroup of k_scc_edge_rows (kCcPiece of gm_components.hip, measured there)
constexpr int kSccLanes = 8;         // lanes per listed vertex in k_scc_pass (measured: 8 / 16 / 32 / 64, profiles/scc.md (c))
constexpr int kSccLongRow = 1024;    // rows of more entries go to k_scc_long (measured: 256 / 1024 / 4096 / never, profiles/scc.md (c))
constexpr int kSccLongBlocks = 32;   // workgroups per row of k_scc_long (kKcLongBlocks)
static_assert(64 % kSccLanes == 0 && kSccPiece % kSccBlock == 0 && kSccPiece / kSccBlock <= 32, "whole groups per wave; a bit per turn of k_scc_compact");

enum : int32_t { kSccDead = 0, kSccAlive = 1, kSccListed = 2, kSccMarked = 3 };

struct SccFlags {      // workspace slot GM_WS_SCC_FLAG; the host reads all of it after every pass
  uint32_t len[2];     // lengths of the two lists
  uint32_t nlong;      // rows the last pass handed to k_scc_long
  uint32_t changed;    // the last forward or backward pass (numbered through the call, from 1) that changed something
  uint32_t nroots;     // roots of all rounds
  uint32_t nedges;     // edges k_scc_compact kept
  uint32_t nused;      // used device slots
  uint32_t unused_;
};

struct SccRows { const int64_t* rowptr; const int32_t* colidx; };
struct SccPeel {       // what a decrement needs
  int32_t* indeg;      // per device id (laying the counters out apart, as KcDeg of gm_kcore.hip does, measured no gain: profiles/scc.md (d))
  int32_t* outdeg;
  int32_t* state;
  int32_t* next;       // the list this pass fills
  uint32_t* next_len;
  uint32_t cap;
};

__device__ __forceinline__ int scc_row_of(const int64_t* __restrict__ rowptr, int lo, int hi, int64_t e) {
  while (hi - lo > 1) {  // the r in [lo, hi) with rowptr[r] <= e < rowptr[r + 1] (given rowptr[lo] <= e < rowptr[hi])
    const int mid = lo + ((hi - lo) >> 1);
    if (rowptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int scc_native(const int32_t* __restrict__ native_of_dev, int dev) { return native_of_dev ? native_of_dev[dev] : dev; }
__device__ __forceinline__ unsigned long long scc_below(int lane) { return (1ull << lane) - 1ull; }  // the lanes before `lane`

// the first position in [lo, end) of row entries whose native id is >= key (upper: > key); a row ascends in native ids
template <bool UPPER>
__device__ __forceinline__ int64_t scc_bound(const int32_t* __restrict__ colidx, const int32_t* __restrict__ native_of_dev, int64_t lo, int64_t end, int key) {
  int64_t hi = end;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int x = scc_native(native_of_dev, colidx[mid]);
    if (UPPER ? x <= key : x < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// the entries of row v that are not v itself
__device__ __forceinline__ int scc_nonloops(SccRows A, const int32_t* __restrict__ native_of_dev, int v) {
  const int64_t at = A.rowptr[v], end = A.rowptr[v + 1];
  const int key = scc_native(native_of_dev, v);
  const int64_t first = scc_bound<false>(A.colidx, native_of_dev, at, end, key);
  return (int)((end - at) - (scc_bound<true>(A.colidx, native_of_dev, first, end, key) - first));
}

// list[old length ...] <- w of the lanes with `hit`: one atomic add per wave; every lane of the wave calls it (kc_append)
__device__ __forceinline__ void scc_append(bool hit, int w, int32_t* __restrict__ list, uint32_t* len, uint32_t cap) {
  const unsigned long long m = __ballot(hit);
  if (m == 0) return;
  const int lane = threadIdx.x & 63, leader = __builtin_ctzll(m);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(len, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, leader);
  const uint32_t at = base + (uint32_t)__popcll(m & scc_below(lane));
  if (hit && at < cap) list[at] = w;
}
// *word += the number of lanes with `hit`, once per wave; every lane of the wave calls it
__device__ __forceinline__ void scc_count(bool hit, uint32_t* word) {
  const unsigned long long m = __ballot(hit);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(word, (uint32_t)__popcll(m));
}

// ---------------- set-up -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSccBlock)
k_scc_init(int32_t* __restrict__ labels, int32_t* __restrict__ state, int32_t* __restrict__ vid, const int32_t* __restrict__ native_of_dev, int n,
           int nparts, int nvertices, SccFlags* flags) {  // (the flags block was cleared before this launch)
  const int v = blockIdx.x * kSccBlock + threadIdx.x;
  const bool used = v < n && (!native_of_dev || native_of_dev[v] >= 0);
  if (v < n) {
    labels[v] = 0;
    state[v] = used ? kSccAlive : kSccDead;
    vid[v] = used ? to_vertex1(scc_native(native_of_dev, v), nparts, nvertices) : 0;
  }
  scc_count(used, &flags->nused);
}

__global__ void __launch_bounds__(kSccBlock)
k_scc_degrees(SccRows OUT, SccRows IN, const int32_t* __restrict__ native_of_dev, int32_t* __restrict__ indeg, int32_t* __restrict__ outdeg, int n) {
  const int v = blockIdx.x * kSccBlock + threadIdx.x;
  if (v >= n) return;
  indeg[v] = scc_nonloops(OUT, native_of_dev, v);
  outdeg[v] = scc_nonloops(IN, native_of_dev, v);
}

// k_cc_edge_rows of gm_components.hip: the rows of a workgroup's first and last edge bound every lane's search
__global__ void __launch_bounds__(kSccBlock)
k_scc_edge_rows(const int64_t* __restrict__ rowptr, int nrows, int64_t nnz, int32_t* __restrict__ row_of_edge) {
  const int64_t first = (int64_t)blockIdx.x * kSccPiece;
  if (first >= nnz) return;
  const int64_t last = first + kSccPiece - 1 < nnz ? first + kSccPiece - 1 : nnz - 1;
  const int rlo = scc_row_of(rowptr, 0, nrows, first);
  const int rhi = scc_row_of(rowptr, rlo, nrows, last);
  for (int64_t e = first + threadIdx.x; e <= last; e += kSccBlock) row_of_edge[e] = scc_row_of(rowptr, rlo, rhi + 1, e);
}

// ---------------- (a) trim -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSccBlock)
k_scc_first_list(int32_t* __restrict__ state, const int32_t* __restrict__ indeg, const int32_t* __restrict__ outdeg, int n, int32_t* __restrict__ list, SccFlags* flags, int cur) {
  const int v = blockIdx.x * kSccBlock + threadIdx.x;
  const bool hit = v < n && state[v] == kSccAlive && (indeg[v] == 0 || outdeg[v] == 0);
  if (hit) state[v] = kSccListed;
  scc_append(hit, v, list, &flags->len[cur], (uint32_t)n);
}

// neighbour x of the dying vertex v loses an entry of deg[]; every lane of the wave calls it
__device__ __forceinline__ void scc_drop(bool valid, int x, int v, int32_t* deg, const SccPeel& P) {
  bool hit = false;
  if (valid && x != v && P.state[x] == kSccAlive) {  // (the look: see the head of this file)
    if (atomicSub(&deg[x], 1) == 1) hit = atomicCAS(&P.state[x], kSccAlive, kSccListed) == kSccAlive;
  }
  scc_append(hit, x, P.next, P.next_len, P.cap);
}

// one of v's two rows, kSccLanes lanes striding over it; v < 0: a group without a vertex.  Every lane of the wave calls it.
__device__ __forceinline__ void scc_walk(SccRows A, int v, int gl, int dir, int32_t* deg, const SccPeel& P, int32_t* __restrict__ long_list,
                                         uint32_t long_cap, SccFlags* flags) {
  int64_t at = 0, end = 0;
  if (v >= 0) {
    at = A.rowptr[v];
    end = A.rowptr[v + 1];
    if (end - at > kSccLongRow) {
      if (gl == 0) {  // (rare by construction: at most 2 * nnz / kSccLongRow times in a call)
        const uint32_t i = atomicAdd(&flags->nlong, 1u);
        if (i < long_cap) { long_list[2 * i] = v; long_list[2 * i + 1] = dir; }
      }
      end = at;
    }
  }
  int turns = (int)((end - at + kSccLanes - 1) / kSccLanes);  // <= kSccLongRow / kSccLanes; the wave's largest, so that every lane stays in the loop
#pragma unroll
  for (int o = 32; o >= kSccLanes; o >>= 1) { const int y = __shfl_xor(turns, o); turns = y > turns ? y : turns; }
  at += gl;
  for (int i = 0; i < turns; i++, at += kSccLanes) {
    const bool valid = at < end;
    scc_drop(valid, valid ? A.colidx[at] : 0, v, deg, P);
  }
}

// label_of = vid: a trim pass (the listed vertices are their own components); label_of = colour: a round's removal pass
__global__ void __launch_bounds__(kSccBlock)
k_scc_pass(const int32_t* __restrict__ list, uint32_t len, SccRows OUT, SccRows IN, SccPeel P, int32_t* __restrict__ labels,
           const int32_t* __restrict__ label_of, int32_t* __restrict__ long_list, uint32_t long_cap, SccFlags* flags, int cur) {
  const uint64_t t = (uint64_t)blockIdx.x * kSccBlock + threadIdx.x, grp = t / kSccLanes;
  const int gl = (int)(t % kSccLanes);
  if (t == 0) flags->len[cur] = 0u;  // (this launch got the length as an argument; the list is the one after next)
  int v = -1;
  if (grp < len) {
    v = list[grp];
    if (gl == 0) { labels[v] = label_of[v]; P.state[v] = kSccDead; }
  }
  scc_walk(IN, v, gl, 0, P.indeg, P, long_list, long_cap, flags);    // v's out-neighbours lose an in-edge
  scc_walk(OUT, v, gl, 1, P.outdeg, P, long_list, long_cap, flags);  // v's in-neighbours lose an out-edge
}

__global__ void __launch_bounds__(kSccBlock)
k_scc_long(const int32_t* __restrict__ long_list, SccRows OUT, SccRows IN, SccPeel P, SccFlags* flags) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) flags->nlong = 0u;  // (this launch got the number as its grid)
  const int v = long_list[2 * blockIdx.x], dir = long_list[2 * blockIdx.x + 1];  // (vertex, adjacency) as scc_walk wrote them
  const SccRows A = dir ? OUT : IN;
  int32_t* deg = dir ? P.outdeg : P.indeg;
  const int64_t end = A.rowptr[v + 1];
  for (int64_t base = A.rowptr[v] + (int64_t)blockIdx.y * kSccBlock; base < end; base += (int64_t)kSccLongBlocks * kSccBlock) {
    const int64_t at = base + threadIdx.x;
    const bool valid = at < end;
    scc_drop(valid, valid ? A.colidx[at] : 0, v, deg, P);
  }
}

// ---------------- (b) a round --------------------------------------------------------------------------------------------------
// the edges u -> w with both ends alive and u != w, in any order: rows[] = w, cols[] = u.  A workgroup takes kSccPiece consecutive
// edges and ONE place for all it keeps (an atomic per wave on the one counter is served one after the other: 10 ns each, measured)
__global__ void __launch_bounds__(kSccBlock)
k_scc_compact(const int32_t* __restrict__ row_of_edge, const int32_t* __restrict__ colidx, int64_t nnz, const int32_t* __restrict__ state,
              int32_t* __restrict__ rows, int32_t* __restrict__ cols, SccFlags* flags) {
  constexpr int kTurns = kSccPiece / kSccBlock, kWaves = kSccBlock / 64;
  __shared__ uint32_t s_at[kTurns * kWaves + 1];  // per (turn, wave): its kept edges, then where they go
  const int64_t first = (int64_t)blockIdx.x * kSccPiece;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t keeps = 0;  // bit i: this thread keeps its edge of turn i
#pragma unroll
  for (int i = 0; i < kTurns; i++) {
    const int64_t e = first + (int64_t)i * kSccBlock + threadIdx.x;
    bool keep = false;
    if (e < nnz) {
      const int w = row_of_edge[e], u = colidx[e];
      keep = u != w && state[u] == kSccAlive && state[w] == kSccAlive;
    }
    keeps |= (uint32_t)keep << i;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_at[i * kWaves + wv] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    for (int j = 0; j < kTurns * kWaves; j++) { const uint32_t c = s_at[j]; s_at[j] = total; total += c; }
    s_at[kTurns * kWaves] = total ? atomicAdd(&flags->nedges, total) : 0u;  // (at most nnz in all: every edge is kept once)
  }
  __syncthreads();
  const uint32_t base = s_at[kTurns * kWaves];
#pragma unroll
  for (int i = 0; i < kTurns; i++) {
    const bool keep = (keeps >> i) & 1u;
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int64_t e = first + (int64_t)i * kSccBlock + threadIdx.x;
      const uint32_t at = base + s_at[i * kWaves + wv] + (uint32_t)__popcll(m & scc_below(lane));
      rows[at] = row_of_edge[e];
      cols[at] = colidx[e];
    }
  }
}

__global__ void __launch_bounds__(kSccBlock)
k_scc_colour(const int32_t* __restrict__ state, const int32_t* __restrict__ vid, int32_t* __restrict__ colour, int n) {
  const int v = blockIdx.x * kSccBlock + threadIdx.x;
  if (v < n && state[v] == kSccAlive) colour[v] = vid[v];
}

__global__ void __launch_bounds__(kSccBlock)
k_scc_forward(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols, int64_t m, const int32_t* __restrict__ state, int32_t* colour,
              uint32_t pass, SccFlags* __restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * kSccBlock + threadIdx.x;
  bool lowered = false;
  if (e < m) {
    const int w = rows[e], u = cols[e];
    if (u != w && state[u] == kSccAlive && state[w] == kSccAlive) {
      const int cu = colour[u];
      // the look of cc_min_into: the word only decreases, so one seen at or below cu -- however old the value seen -- needs no atomic
      if (__hip_atomic_load(&colour[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > cu) lowered = atomicMin(&colour[w], cu) > cu;
    }
  }
  if (__any(lowered) && (threadIdx.x & 63) == 0) flags->changed = pass;  // (every wave stores the same value)
}

__global__ void __launch_bounds__(kSccBlock)
k_scc_roots(int32_t* __restrict__ state, const int32_t* __restrict__ vid, const int32_t* __restrict__ colour, int n, SccFlags* flags) {
  const int v = blockIdx.x * kSccBlock + threadIdx.x;
  const bool root = v < n && state[v] == kSccAlive && colour[v] == vid[v];
  if (root) state[v] = kSccMarked;
  scc_count(root, &flags->nroots);
}

__global__ void __launch_bounds__(kSccBlock)
k_scc_backward(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols, int64_t m, int32_t* state, const int32_t* __restrict__ colour,
               uint32_t pass, SccFlags* __restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * kSccBlock + threadIdx.x;
  bool marked = false;
  if (e < m) {
    const int w = rows[e], u = cols[e];
    marked = state[w] == kSccMarked && state[u] == kSccAlive && colour[u] == colour[w];
    if (marked) state[u] = kSccMarked;  // (several lanes may store the same value)
  }
  if (__any(marked) && (threadIdx.x & 63) == 0) flags->changed = pass;
}

__global__ void __launch_bounds__(kSccBlock)
k_scc_gather(const int32_t* __restrict__ state, int n, int32_t* __restrict__ list, SccFlags* flags, int cur) {
  const int v = blockIdx.x * kSccBlock + threadIdx.x;
  scc_append(v < n && state[v] == kSccMarked, v, list, &flags->len[cur], (uint32_t)n);
}

static inline unsigned scc_grid(int64_t n, int per_block = kSccBlock) { return n > 0 ? (unsigned)((n + per_block - 1) / per_block) : 1u; }  // (no empty grid)
static inline size_t scc_pad(size_t bytes) { return (bytes + 63) / 64 * 64; }

// ev[0..3]: created and destroyed by the caller, whatever this returns
static int strong_components(gm_graph_t* g, int32_t* d_labels, int32_t* h_ncomponents, hipStream_t s, hipEvent_t* ev) {
  const gm_csr_t& O = g->out.view;
  const gm_csr_t& I = g->in.view;
  const int n = O.nrows;
  const int64_t nnz = O.nnz;
  const SccRows OUT = {O.rowptr, O.colidx}, IN = {I.rowptr, I.colidx};
  const size_t long_cap = (size_t)((nnz + I.nnz) / kSccLongRow) + 2;  // (vertex, adjacency) pairs a pass can hand over
  int rc;
  void* p = nullptr;
  if ((rc = gm_graph_workspace(g, GM_WS_SCC_FLAG, 64, &p))) return rc;
  SccFlags* flags = (SccFlags*)p;
  SccPeel P;
  const size_t vbytes = scc_pad((size_t)n * 4);
  if ((rc = gm_graph_workspace(g, GM_WS_SCC_STATE, 7 * vbytes + scc_pad(long_cap * 8) + 64, &p))) return rc;
  char* at = (char*)p;
  P.indeg = (int32_t*)at; at += vbytes;
  P.outdeg = (int32_t*)at; at += vbytes;
  int32_t* vid = (int32_t*)at; at += vbytes;
  int32_t* state = (int32_t*)at; at += vbytes;
  int32_t* colour = (int32_t*)at; at += vbytes;
  int32_t* list[2];
  list[0] = (int32_t*)at; at += vbytes;
  list[1] = (int32_t*)at; at += vbytes;
  int32_t* long_list = (int32_t*)at;
  const size_t ebytes = scc_pad((size_t)nnz * 4);
  if ((rc = gm_graph_workspace(g, GM_WS_SCC_EDGES, 3 * ebytes + 64, &p))) return rc;
  int32_t* row_of_edge = (int32_t*)p;
  int32_t* kept_rows = (int32_t*)((char*)p + ebytes);
  int32_t* kept_cols = (int32_t*)((char*)p + 2 * ebytes);
  const int32_t* native_of_dev = g->native_of_dev;
  P.state = state;
  P.cap = (uint32_t)n;

  // gm_graph_last_stats afterwards: send_ms = set-up and the first trim, spmv_ms = the rounds with their trims, apply_ms = what
  // remains; iterations = rounds, spmv_launches = passes (trim lists, forward and backward passes; not the removal passes)
  gm_run_stats_t st;
  memset(&st, 0, sizeof(st));
  // the flags land in the graph's pinned block, as in gm_kcore.hip (measured there)
  SccFlags h_own;
  SccFlags& h = g->pinned_flag ? *(SccFlags*)g->pinned_flag : h_own;
  memset(&h, 0, sizeof(h));
  auto read_flags = [&]() -> int {
    GM_TRY_HIP(hipMemcpyAsync(&h, flags, sizeof(h), hipMemcpyDeviceToHost, s));
    GM_TRY_HIP(hipStreamSynchronize(s));
    return GM_OK;
  };
  int cur = 0;
  // one pass over list[cur] (len > 0 entries), the long rows it hands over included; afterwards list[cur] is what it listed
  auto pass_over_list = [&](uint32_t len, const int32_t* label_of) -> int {
    P.next = list[cur ^ 1];
    P.next_len = &flags->len[cur ^ 1];
    hipLaunchKernelGGL(k_scc_pass, dim3(scc_grid((int64_t)len * kSccLanes)), dim3(kSccBlock), 0, s, (const int32_t*)list[cur], len, OUT, IN, P, d_labels,
                       label_of, long_list, (uint32_t)long_cap, flags, cur);
    int r;
    if ((r = read_flags())) return r;
    if (h.nlong > 0) {
      const uint32_t nlong = h.nlong < (uint32_t)long_cap ? h.nlong : (uint32_t)long_cap;
      hipLaunchKernelGGL(k_scc_long, dim3(nlong, kSccLongBlocks), dim3(kSccBlock), 0, s, (const int32_t*)long_list, OUT, IN, P, flags);
      if ((r = read_flags())) return r;
    }
    cur ^= 1;
    return GM_OK;
  };
  int64_t alive = 0, trimmed = 0;  // (the lists' lengths were added once per wave; one more word for all trimmed vertices would be one atomic
                                   // per wave of k_scc_pass on one address: measured, 25 ms of a 60 ms call on RMAT-22, profiles/scc.md)
  // every listed vertex dies in its pass and enters no list again: at most n passes in the whole call
  auto trim_to_fixpoint = [&]() -> int {
    for (uint32_t len = h.len[cur]; len > 0; len = h.len[cur]) {
      int r;
      if ((r = pass_over_list(len, vid))) return r;
      st.spmv_launches++;
      alive -= len;
      trimmed += len;
    }
    return GM_OK;
  };

  GM_TRY_HIP(hipEventRecord(ev[0], s));
  GM_TRY_HIP(hipMemsetAsync(flags, 0, 64, s));
  hipLaunchKernelGGL(k_scc_init, dim3(scc_grid(n)), dim3(kSccBlock), 0, s, d_labels, state, vid, native_of_dev, n, g->desc.nparts, g->desc.nvertices, flags);
  hipLaunchKernelGGL(k_scc_degrees, dim3(scc_grid(n)), dim3(kSccBlock), 0, s, OUT, IN, native_of_dev, P.indeg, P.outdeg, n);
  if (nnz > 0) hipLaunchKernelGGL(k_scc_edge_rows, dim3(scc_grid(nnz, kSccPiece)), dim3(kSccBlock), 0, s, O.rowptr, n, nnz, row_of_edge);
  hipLaunchKernelGGL(k_scc_first_list, dim3(scc_grid(n)), dim3(kSccBlock), 0, s, state, P.indeg, P.outdeg, n, list[cur], flags, cur);
  if ((rc = read_flags())) return rc;
  alive = (int64_t)h.nused;
  if ((rc = trim_to_fixpoint())) return rc;
  GM_TRY_HIP(hipEventRecord(ev[1], s));

  const int32_t* rows = row_of_edge;
  const int32_t* cols = O.colidx;
  int64_t m = nnz;
  uint32_t pass = 0;
  for (int64_t round = 1; alive > 0 && round <= (int64_t)n; round++) {  // a round removes at least the SCC of the smallest alive id
    st.iterations = (int32_t)round;
    if (round == 1) {  // the edge passes run over the edges alive after the first trim (measured: 21 against 32 ms on RMAT-22, profiles/scc.md (b))
      hipLaunchKernelGGL(k_scc_compact, dim3(scc_grid(nnz, kSccPiece)), dim3(kSccBlock), 0, s, (const int32_t*)row_of_edge, O.colidx, nnz, (const int32_t*)state,
                         kept_rows, kept_cols, flags);
      if ((rc = read_flags())) return rc;
      rows = kept_rows;
      cols = kept_cols;
      m = (int64_t)h.nedges;
    }
    hipLaunchKernelGGL(k_scc_colour, dim3(scc_grid(n)), dim3(kSccBlock), 0, s, (const int32_t*)state, (const int32_t*)vid, colour, n);
    for (int64_t i = 0; i <= (int64_t)n; i++) {  // a pass that changes something lowers a colour: at most n of them, and the one that confirms
      pass++;
      hipLaunchKernelGGL(k_scc_forward, dim3(scc_grid(m)), dim3(kSccBlock), 0, s, rows, cols, m, (const int32_t*)state, colour, pass, flags);
      if ((rc = read_flags())) return rc;
      st.spmv_launches++;
      if (h.changed != pass) break;
    }
    hipLaunchKernelGGL(k_scc_roots, dim3(scc_grid(n)), dim3(kSccBlock), 0, s, state, (const int32_t*)vid, (const int32_t*)colour, n, flags);
    for (int64_t i = 0; i <= (int64_t)n; i++) {  // a pass that changes something sets a mark
      pass++;
      hipLaunchKernelGGL(k_scc_backward, dim3(scc_grid(m)), dim3(kSccBlock), 0, s, rows, cols, m, state, (const int32_t*)colour, pass, flags);
      if ((rc = read_flags())) return rc;
      st.spmv_launches++;
      if (h.changed != pass) break;
    }
    hipLaunchKernelGGL(k_scc_gather, dim3(scc_grid(n)), dim3(kSccBlock), 0, s, (const int32_t*)state, n, list[cur], flags, cur);
    if ((rc = read_flags())) return rc;
    const uint32_t removed = h.len[cur];  // (at least the round's roots)
    if (removed > 0 && (rc = pass_over_list(removed, colour))) return rc;
    alive -= removed;
    if ((rc = trim_to_fixpoint())) return rc;
  }
  GM_TRY_HIP(hipEventRecord(ev[2], s));
  if ((rc = read_flags())) return rc;
  GM_TRY_HIP(hipEventRecord(ev[3], s));
  GM_TRY_HIP(hipEventSynchronize(ev[3]));
  GM_TRY_HIP(hipGetLastError());
  if (h_ncomponents) *h_ncomponents = (int32_t)(trimmed + (int64_t)h.nroots);
  GM_TRY_HIP(hipEventElapsedTime(&st.send_ms, ev[0], ev[1]));
  GM_TRY_HIP(hipEventElapsedTime(&st.spmv_ms, ev[1], ev[2]));
  GM_TRY_HIP(hipEventElapsedTime(&st.apply_ms, ev[2], ev[3]));
  st.total_ms = st.send_ms + st.spmv_ms + st.apply_ms;
  g->stats = st;
  return GM_OK;
}

static int run_strong_components(gm_graph_t* g, int32_t* d_labels, int32_t* h_ncomponents, hipStream_t s) {
  if (g->out.view.nrows <= 0) { if (h_ncomponents) *h_ncomponents = 0; return GM_OK; }
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  int rc = GM_OK;
  for (hipEvent_t& e : ev) {
    if (rc == GM_OK && hipEventCreate(&e) != hipSuccess) { set_error("gm_run_strong_components: hipEventCreate failed"); rc = GM_ERR_HIP; }
  }
  if (rc == GM_OK) rc = strong_components(g, d_labels, h_ncomponents, s, ev);
  for (hipEvent_t& e : ev) if (e) (void)hipEventDestroy(e);
  return rc;
}

}  // namespace gm

extern "C" int gm_run_strong_components(gm_graph_t* g, int32_t* d_labels, int32_t* h_ncomponents, gm_stream_t stream) {
  // argument errors first: nothing on the GPU is touched
  if (!g || !d_labels) { gm::set_error("gm_run_strong_components: null graph or output array"); return GM_ERR_INVALID; }
  const gm_graph_desc_t& d = g->desc;
  if (d.row_lo != 0 || d.row_hi != d.ndevice || d.nshards > 1 || g->xfn != nullptr) {
    gm::set_error("gm_run_strong_components: whole graphs only (no shards, no row ranges)");
    return GM_ERR_UNSUPPORTED;
  }
  if (!g->out.present || !g->in.present) {
    gm::set_error("gm_run_strong_components: needs both adjacencies (a graph built with GM_DIR_OUT | GM_DIR_IN)");
    return GM_ERR_UNSUPPORTED;
  }
  return gm::run_strong_components(g, d_labels, h_ncomponents, (hipStream_t)stream);
}
