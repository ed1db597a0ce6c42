// gm_kcore.hip -- k-core decomposition by peeling, exact integers.
//
// core[v] = the largest k such that v lies in a subgraph in which every vertex has at least k neighbours, in the SIMPLE UNDIRECTED
// graph under the edge list: directions are ignored, self-loops dropped, duplicate edges and antiparallel pairs count once.  A vertex
// without neighbours has 0; kmax is the largest core number.  One adjacency is read (GM_DIR_OUT when the graph has it, else
// GM_DIR_IN): every edge stands in it once.
//
// (a) The simple adjacency, built once per call into workspace (rowptr int64, entries int32 device ids, at most 2 * nnz of them).
// The graph's CSR holds device ids in ascending NATIVE column order, duplicates adjacent.  For every distinct non-loop entry
// (row r, column c): c is a neighbour of r (a "forward" entry); r is a neighbour of c (a "reverse" entry) unless row c holds r itself
// -- a binary search of row c on native ids -- because then row c's own forward entry supplies it.
//   k_kc_init    deg[v] = 0, core[v] = -1 (alive) for used slots and 0 for unused ones (never alive, never counted), flags cleared
//   k_kc_mark    lane = edge: finds (r, c), decides forward / reverse and takes a place in the target row: slot = the value that
//                atomicAdd(&deg[row], count) returns, so deg[] ends as the simple degree and a place costs no second pass of atomics.
//                Edges of one wave lie in consecutive rows: the forward entries of a row take ONE atomic per wave (segments of equal
//                r), so a giant row costs one atomic per 64 entries; a reverse entry takes one of its own.  deg[] is laid out so that
//                neighbouring device ids do not share a cache line (KcDeg): the hubs of a degree-ranked order would queue behind
//                each other's atomics otherwise, here and in the peel
//   k_kc_scan_*  rowptr = exclusive prefix sums of deg: block sums, one workgroup over the block sums, the rows of each block
//   k_kc_place   lane = edge: entries[rowptr[row] + slot] = neighbour.  The order inside a row is the order of arrival; nothing reads it
// (b) The peel.  deg[] is changed by atomics only and only ever decreases from here on; core[] is the caller's array; two frontier
// lists of at most n vertices each (every vertex enters a list exactly once in the whole call).
//   k_kc_level_min   k = the smallest deg among alive vertices, and their number (a workgroup reduces, then one atomic each)
//   k_kc_level_list  appends the alive vertices with deg == k (one atomic add per wave: ballot + popcount).  k jumps over empty
//                    levels, so there are as many levels as distinct core numbers
//   k_kc_pass        a group of kKcLanes lanes per listed vertex v: core[v] = k; the group strides over v's row; for each neighbour w
//                    seen with deg[w] > k: old = atomicSub(&deg[w], 1), and the one thread that gets old == k + 1 appends w to the
//                    next list.  A row of more than kKcLongRow entries is handed to
//   k_kc_long        a vertex per blockIdx.x, kKcLongBlocks workgroups striding over its row: the same step, lane = entry
// The host reads the flags block (32 bytes) after each level's two kernels (k, alive, the list's length) and after each pass (the
// next list's length, the number of long rows handed over); kmax rides in the same block, so the last read brings it.
// Bounds: a level with alive vertices lists at least one (the minimum is attained) and every listed vertex dies in its pass, so at
// most n levels and n passes; the loops in kernels run over a row's length or a list's length.
//
// Memory model.  Inside one launch a plain load may return an older value than another workgroup has written (a CU's L1, another
// XCD's L2); atomics are coherent.  Nothing here needs more.  deg[] only decreases during the peel, so an older deg[w] is a larger
// one: the look `deg[w] > k` (a load past the CU's L1) can be wrong only towards "still above k", which costs one atomic on a vertex
// that is dead or listed already -- its deg is at or below k, the atomic returns at most k, nobody is appended, and a dead vertex's
// deg is never read again.  A look that says deg[w] <= k is true now as well, and such a w is dead or listed: skipping it is right.
// Who appends w is decided by the value the atomic returns: deg[w] passes from k + 1 to k exactly once.  A vertex listed by
// k_kc_level_list has deg == k and is never seen at k + 1 again.  core[] and the list lengths are read across kernel boundaries only
// (the lengths by the host, which passes them as arguments).  No kernel waits for another wave or workgroup, nothing is retried,
// no kernel is persistent or cooperative.
// Measurements and the choices taken from them: profiles/kcore.md.
#include <limits.h>
#include <string.h>

#include "gm_internal.hpp"

namespace gm {

constexpr int kKcBlock = 256;       // (not measured: the block size of gm_triangles.hip and gm_components.hip)
constexpr int kKcPiece = 4096;      // edges per workgroup of k_kc_mark (kCcPiece of gm_components.hip, measured there)
constexpr int kKcLanes = 64;         // lanes per listed vertex in k_kc_pass (measured: 8 / 16 / 32 / 64, profiles/kcore.md)
constexpr int kKcLongRow = 1024;    // rows of more entries are peeled by k_kc_long (measured: 1024 / 4096 / 16384)
constexpr int kKcSpreadLog2 = 10;   // deg[] is laid out 2^this device ids apart (KcDeg; measured: 0 / 10)
constexpr int kKcLongBlocks = 32;   // workgroups per vertex of k_kc_long
constexpr int kKcScanItems = 8;     // degrees per thread of the scan kernels
constexpr int kKcScanBlock = kKcBlock * kKcScanItems;
constexpr int kKcLevelGrid = 1024;  // workgroups of k_kc_level_min at the most: one pair of atomics each
static_assert(64 % kKcLanes == 0 && kKcLanes >= 1, "whole groups per wave");

struct KcFlags {       // workspace slot GM_WS_KC_FLAG
  uint32_t len[2];     // lengths of the two frontier lists
  uint32_t nlong;      // vertices the last pass handed to k_kc_long
  uint32_t kmin[2];    // smallest degree among alive vertices, level by level in turn
  uint32_t alive[2];   // their number
  uint32_t kmax;       // k of the last level that had alive vertices
};

// deg[] of vertex v.  Neighbouring device ids do not share a cache line: with the degree-ranked device order the busiest vertices
// have the smallest ids, and atomics to one LINE are served one after the other like atomics to one word, so sixteen hubs in a
// line would queue behind each other.  v -> (v mod 2^shift) * stride + v / 2^shift (shift 0: the identity).
struct KcDeg {
  int32_t* p;
  int mask, shift, stride;
  __device__ __forceinline__ int32_t* at(int v) const { return p + (int64_t)(v & mask) * stride + (v >> shift); }
};

__device__ __forceinline__ int kc_row_of(const int64_t* __restrict__ rowptr, int lo, int hi, int64_t e) {
  while (hi - lo > 1) {  // the r in [lo, hi) with rowptr[r] <= e < rowptr[r + 1] (given rowptr[lo] <= e < rowptr[hi])
    const int mid = lo + ((hi - lo) >> 1);
    if (rowptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int kc_native(const int32_t* __restrict__ native_of_dev, int dev) { return native_of_dev ? native_of_dev[dev] : dev; }
__device__ __forceinline__ unsigned long long kc_below(int lane) { return (1ull << lane) - 1ull; }  // the lanes before `lane`

// does row c of A hold column r?  (a row ascends in native ids; equal device ids are equal native ids)
__device__ __forceinline__ bool kc_row_holds(const gm_csr_t& A, const int32_t* __restrict__ native_of_dev, int c, int r) {
  const int key = kc_native(native_of_dev, r);
  int64_t lo = A.rowptr[c];
  const int64_t end = A.rowptr[c + 1];
  int64_t hi = end;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (kc_native(native_of_dev, A.colidx[mid]) < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && A.colidx[lo] == r;
}

// list[old length ...] <- w of the lanes with `hit`: one atomic add per wave; every lane of the wave calls it.  cap = the list's size
__device__ __forceinline__ void kc_append(bool hit, int w, int32_t* __restrict__ list, uint32_t* len, uint32_t cap) {
  const unsigned long long m = __ballot(hit);
  if (m == 0) return;
  const int lane = threadIdx.x & 63, leader = __builtin_ctzll(m);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(len, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, leader);
  const uint32_t at = base + (uint32_t)__popcll(m & kc_below(lane));
  if (hit && at < cap) list[at] = w;
}

__global__ void __launch_bounds__(kKcBlock)
k_kc_init(int32_t* __restrict__ core, int32_t* __restrict__ deg, int ndeg, const int32_t* __restrict__ native_of_dev, int n, KcFlags* __restrict__ flags) {
  const int v = blockIdx.x * kKcBlock + threadIdx.x;
  if (v == 0) {
    flags->len[0] = flags->len[1] = flags->nlong = 0u;
    flags->kmin[0] = flags->kmin[1] = UINT_MAX;
    flags->alive[0] = flags->alive[1] = 0u;
    flags->kmax = 0u;
  }
  if (v < ndeg) deg[v] = 0;  // (by position: ndeg >= n)
  if (v >= n) return;
  core[v] = (!native_of_dev || native_of_dev[v] >= 0) ? -1 : 0;
}

// ---------------- (a) the simple adjacency ----------------------------------------------------------------------------------
// A workgroup's kKcPiece consecutive edges lie in few rows: the rows of its first and last edge are searched in all of rowptr, every
// lane then searches between the two (k_cc_edge_rows of gm_components.hip).  The loop runs the same number of times in every lane.
__global__ void __launch_bounds__(kKcBlock)
k_kc_mark(gm_csr_t A, const int32_t* __restrict__ native_of_dev, KcDeg deg, int32_t* __restrict__ row_of_edge, int32_t* __restrict__ fslot,
          int32_t* __restrict__ rslot) {
  const int64_t first = (int64_t)blockIdx.x * kKcPiece;
  if (first >= A.nnz) return;
  const int64_t last = first + kKcPiece - 1 < A.nnz ? first + kKcPiece - 1 : A.nnz - 1;
  const int rlo = kc_row_of(A.rowptr, 0, A.nrows, first);
  const int rhi = kc_row_of(A.rowptr, rlo, A.nrows, last);
  const int lane = threadIdx.x & 63;
  for (int64_t base = first; base <= last; base += kKcBlock) {
    const int64_t e = base + threadIdx.x;
    const bool valid = e <= last;
    int r = -1, c = -1;
    bool keep = false;
    if (valid) {
      r = kc_row_of(A.rowptr, rlo, rhi + 1, e);
      c = A.colidx[e];
      keep = c != r && (e == A.rowptr[r] || A.colidx[e - 1] != c);  // no loop, and the first of a run of duplicates
    }
    const bool rev = keep && !kc_row_holds(A, native_of_dev, c, r);
    // forward entries: the lanes of a wave that share r are neighbours; the first of them acts for all
    const int before = __shfl_up(r, 1);
    const unsigned long long heads = __ballot(lane == 0 || before != r), keeps = __ballot(keep);
    const int seg_lo = 63 - __builtin_clzll(heads & (kc_below(lane) | (1ull << lane)));
    const unsigned long long after = heads & ~(kc_below(lane) | (1ull << lane));
    const unsigned long long seg = (after ? kc_below(__builtin_ctzll(after)) : ~0ull) & ~kc_below(seg_lo);
    int fbase = 0;
    if (lane == seg_lo && (keeps & seg)) fbase = atomicAdd(deg.at(r), __popcll(keeps & seg));
    fbase = __shfl(fbase, seg_lo);
    const int fs = keep ? fbase + __popcll(keeps & seg & kc_below(lane)) : -1;
    // reverse entries: one atomic each (lanes of a wave that share c taking one together measured no gain: profiles/kcore.md)
    const int rs = rev ? atomicAdd(deg.at(c), 1) : -1;
    if (valid) { row_of_edge[e] = r; fslot[e] = fs; rslot[e] = rs; }
  }
}

// inclusive prefix sum of x over the workgroup; *total = the workgroup's sum.  Every thread calls it.
__device__ __forceinline__ int64_t kc_block_scan(int64_t x, int64_t* total) {
  __shared__ int64_t s_w[kKcBlock / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int64_t y = __shfl_up(x, o); if (lane >= o) x += y; }
  __syncthreads();  // (the previous call's readers are done)
  if (lane == 63) s_w[wv] = x;
  __syncthreads();
  int64_t t = 0;
#pragma unroll
  for (int w = 0; w < kKcBlock / 64; w++) { if (w < wv) x += s_w[w]; t += s_w[w]; }
  *total = t;
  return x;
}
__global__ void __launch_bounds__(kKcBlock)
k_kc_scan_sums(KcDeg deg, int n, int64_t* __restrict__ bsum) {
  const int64_t i0 = (int64_t)blockIdx.x * kKcScanBlock + (int64_t)threadIdx.x * kKcScanItems;
  int64_t x = 0;
#pragma unroll
  for (int j = 0; j < kKcScanItems; j++) if (i0 + j < n) x += *deg.at((int)(i0 + j));
  int64_t total;
  kc_block_scan(x, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
// one workgroup: bsum[b] <- the sum of the blocks before b; rowptr[n] <- the sum of all
__global__ void __launch_bounds__(kKcBlock)
k_kc_scan_top(int64_t* __restrict__ bsum, int nb, int64_t* __restrict__ rowptr_end) {
  int64_t running = 0;
  for (int base = 0; base < nb; base += kKcBlock) {
    const int b = base + threadIdx.x;
    const int64_t x = b < nb ? bsum[b] : 0;
    int64_t total;
    const int64_t incl = kc_block_scan(x, &total);
    if (b < nb) bsum[b] = running + incl - x;
    running += total;
  }
  if (threadIdx.x == 0) *rowptr_end = running;
}
__global__ void __launch_bounds__(kKcBlock)
k_kc_scan_write(KcDeg deg, int n, const int64_t* __restrict__ bsum, int64_t* __restrict__ rowptr) {
  const int64_t i0 = (int64_t)blockIdx.x * kKcScanBlock + (int64_t)threadIdx.x * kKcScanItems;
  int32_t d[kKcScanItems];
  int64_t x = 0;
#pragma unroll
  for (int j = 0; j < kKcScanItems; j++) { d[j] = i0 + j < n ? *deg.at((int)(i0 + j)) : 0; x += d[j]; }
  int64_t total;
  int64_t at = bsum[blockIdx.x] + kc_block_scan(x, &total) - x;
#pragma unroll
  for (int j = 0; j < kKcScanItems; j++) { if (i0 + j < n) rowptr[i0 + j] = at; at += d[j]; }
}

__global__ void __launch_bounds__(kKcBlock)
k_kc_place(int64_t nnz, const int32_t* __restrict__ colidx, const int32_t* __restrict__ row_of_edge, const int32_t* __restrict__ fslot,
           const int32_t* __restrict__ rslot, const int64_t* __restrict__ rowptr, int32_t* __restrict__ entries) {
  const int64_t e = (int64_t)blockIdx.x * kKcBlock + threadIdx.x;
  if (e >= nnz) return;
  const int fs = fslot[e], rs = rslot[e];
  if (fs < 0) return;  // (no reverse entry without a forward one)
  const int r = row_of_edge[e], c = colidx[e];
  entries[rowptr[r] + fs] = c;
  if (rs >= 0) entries[rowptr[c] + rs] = r;
}

// ---------------- (b) the peel ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kKcBlock)
k_kc_level_min(const int32_t* __restrict__ core, KcDeg deg, int n, KcFlags* flags, int slot) {
  __shared__ uint32_t s_min[kKcBlock / 64], s_cnt[kKcBlock / 64];
  uint32_t mn = UINT_MAX, cnt = 0;
  for (int64_t v = (int64_t)blockIdx.x * kKcBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kKcBlock) {
    if (core[v] == -1) {
      const uint32_t d = (uint32_t)*deg.at((int)v);
      mn = d < mn ? d : mn;
      cnt++;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t y = (uint32_t)__shfl_xor((int)mn, o);
    mn = y < mn ? y : mn;
    cnt += (uint32_t)__shfl_xor((int)cnt, o);
  }
  if ((threadIdx.x & 63) == 0) { s_min[threadIdx.x >> 6] = mn; s_cnt[threadIdx.x >> 6] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kKcBlock / 64; w++) { mn = s_min[w] < mn ? s_min[w] : mn; cnt += s_cnt[w]; }
    if (cnt) {
      atomicAdd(&flags->alive[slot], cnt);
      // the look of gm_components.hip: the word only decreases, so one seen at or below mn needs no atomic
      if (__hip_atomic_load(&flags->kmin[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mn) atomicMin(&flags->kmin[slot], mn);
    }
  }
}

__global__ void __launch_bounds__(kKcBlock)
k_kc_level_list(const int32_t* __restrict__ core, KcDeg deg, int n, int32_t* __restrict__ list, KcFlags* flags, int slot, int cur) {
  const int v = blockIdx.x * kKcBlock + threadIdx.x;
  const uint32_t k = flags->kmin[slot];  // (written by the launch before this one)
  if (v == 0) {  // the other pair of words is the next level's
    flags->kmin[slot ^ 1] = UINT_MAX;
    flags->alive[slot ^ 1] = 0u;
    if (flags->alive[slot]) flags->kmax = k;
  }
  const bool hit = v < n && core[v] == -1 && (uint32_t)*deg.at(v) == k;
  kc_append(hit, v, list, &flags->len[cur], (uint32_t)n);
}

// one step of the peel for neighbour w of a vertex that has just got core number k; every lane of the wave calls it
__device__ __forceinline__ void kc_drop(bool valid, int w, int k, KcDeg deg, int32_t* __restrict__ next, uint32_t* next_len, uint32_t cap) {
  bool hit = false;
  if (valid) {
    int32_t* d = deg.at(w);
    if (__hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > k) hit = atomicSub(d, 1) == k + 1;
  }
  kc_append(hit, w, next, next_len, cap);
}

__global__ void __launch_bounds__(kKcBlock)
k_kc_pass(const int32_t* __restrict__ list, uint32_t len, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ entries, KcDeg deg,
          int32_t* __restrict__ core, int k, int32_t* __restrict__ next, int32_t* __restrict__ long_list, uint32_t long_cap, KcFlags* flags, int cur,
          int n) {
  const uint64_t t = (uint64_t)blockIdx.x * kKcBlock + threadIdx.x, grp = t / kKcLanes;
  const int gl = (int)(t % kKcLanes);
  if (t == 0) flags->len[cur] = 0u;  // (this launch got the length as an argument; the list is the one after next)
  int64_t at = 0, end = 0;
  if (grp < len) {
    const int v = list[grp];
    at = rowptr[v];
    end = rowptr[v + 1];
    if (gl == 0) core[v] = k;
    if (end - at > kKcLongRow) {
      if (gl == 0) {  // (rare by construction: at most 2 * nnz / kKcLongRow times in a call)
        const uint32_t i = atomicAdd(&flags->nlong, 1u);
        if (i < long_cap) long_list[i] = v;
      }
      end = at;
    }
  }
  int turns = (int)((end - at + kKcLanes - 1) / kKcLanes);  // <= kKcLongRow / kKcLanes; the wave's largest, so that every lane stays in the loop
#pragma unroll
  for (int o = 32; o >= kKcLanes; o >>= 1) { const int y = __shfl_xor(turns, o); turns = y > turns ? y : turns; }
  at += gl;
  for (int i = 0; i < turns; i++, at += kKcLanes) {
    const bool valid = at < end;
    kc_drop(valid, valid ? entries[at] : 0, k, deg, next, &flags->len[cur ^ 1], (uint32_t)n);
  }
}

__global__ void __launch_bounds__(kKcBlock)
k_kc_long(const int32_t* __restrict__ long_list, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ entries, KcDeg deg, int k,
          int32_t* __restrict__ next, KcFlags* flags, int cur, int n) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) flags->nlong = 0u;  // (this launch got the number as its grid)
  const int v = long_list[blockIdx.x];
  const int64_t end = rowptr[v + 1];
  for (int64_t base = rowptr[v] + (int64_t)blockIdx.y * kKcBlock; base < end; base += (int64_t)kKcLongBlocks * kKcBlock) {
    const int64_t at = base + threadIdx.x;
    const bool valid = at < end;
    kc_drop(valid, valid ? entries[at] : 0, k, deg, next, &flags->len[cur ^ 1], (uint32_t)n);
  }
}

static inline unsigned kc_grid(int64_t n, int per_block = kKcBlock) { return (unsigned)((n + per_block - 1) / per_block); }
static inline size_t kc_pad(size_t bytes) { return (bytes + 63) / 64 * 64; }

static int run_kcore(gm_graph_t* g, int32_t* d_core, int32_t* h_kmax, hipStream_t s) {
  const gm_csr_t& A = g->out.present ? g->out.view : g->in.view;  // either adjacency holds every edge once
  const int n = A.nrows;
  const int64_t nnz = A.nnz;
  if (n <= 0) { if (h_kmax) *h_kmax = 0; return GM_OK; }
  const int nb = (int)kc_grid(n, kKcScanBlock);
  const size_t long_cap = (size_t)(2 * nnz / kKcLongRow) + 1;
  int rc;
  void* p = nullptr;
  if ((rc = gm_graph_workspace(g, GM_WS_KC_FLAG, 64, &p))) return rc;
  KcFlags* flags = (KcFlags*)p;
  const size_t vbytes = kc_pad((size_t)n * 4);
  KcDeg deg;
  deg.shift = kKcSpreadLog2;
  deg.mask = (1 << kKcSpreadLog2) - 1;
  deg.stride = (((n >> kKcSpreadLog2) + 1) + 15) / 16 * 16;  // whole lines, so that two ids a stride apart never share one
  const size_t ndeg = (size_t)deg.stride << kKcSpreadLog2;  // positions: at most n + 17 * 2^kKcSpreadLog2
  const size_t dbytes = kc_pad(ndeg * 4);
  if ((rc = gm_graph_workspace(g, GM_WS_KC_STATE, dbytes + 2 * vbytes + kc_pad(long_cap * 4) + kc_pad((size_t)nb * 8) + 64, &p))) return rc;
  deg.p = (int32_t*)p;
  int32_t* list[2] = {(int32_t*)((char*)p + dbytes), (int32_t*)((char*)p + dbytes + vbytes)};
  int32_t* long_list = (int32_t*)((char*)p + dbytes + 2 * vbytes);
  int64_t* bsum = (int64_t*)((char*)long_list + kc_pad(long_cap * 4));
  const size_t rbytes = kc_pad((size_t)(n + 1) * 8), ebytes = kc_pad((size_t)nnz * 4);
  if ((rc = gm_graph_workspace(g, GM_WS_KC_ADJ, rbytes + 5 * ebytes + 64, &p))) return rc;
  int64_t* rowptr = (int64_t*)p;
  int32_t* entries = (int32_t*)((char*)p + rbytes);  // 2 * nnz at the most
  int32_t* row_of_edge = (int32_t*)((char*)p + rbytes + 2 * ebytes);
  int32_t* fslot = (int32_t*)((char*)p + rbytes + 3 * ebytes);
  int32_t* rslot = (int32_t*)((char*)p + rbytes + 4 * ebytes);
  const int32_t* native_of_dev = g->native_of_dev;

  // gm_graph_last_stats afterwards: send_ms = the adjacency build, spmv_ms = the peel, apply_ms = the finish;
  // iterations = peel passes, spmv_launches = levels
  gm_run_stats_t st;
  memset(&st, 0, sizeof(st));
  hipEvent_t ev[4];
  for (hipEvent_t& e : ev) GM_TRY_HIP(hipEventCreate(&e));
  GM_TRY_HIP(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(k_kc_init, dim3(kc_grid((int64_t)ndeg)), dim3(kKcBlock), 0, s, d_core, deg.p, (int)ndeg, native_of_dev, n, flags);
  if (nnz > 0) hipLaunchKernelGGL(k_kc_mark, dim3(kc_grid(nnz, kKcPiece)), dim3(kKcBlock), 0, s, A, native_of_dev, deg, row_of_edge, fslot, rslot);
  hipLaunchKernelGGL(k_kc_scan_sums, dim3(nb), dim3(kKcBlock), 0, s, deg, n, bsum);
  hipLaunchKernelGGL(k_kc_scan_top, dim3(1), dim3(kKcBlock), 0, s, bsum, nb, rowptr + n);
  hipLaunchKernelGGL(k_kc_scan_write, dim3(nb), dim3(kKcBlock), 0, s, deg, n, (const int64_t*)bsum, rowptr);
  if (nnz > 0)
    hipLaunchKernelGGL(k_kc_place, dim3(kc_grid(nnz)), dim3(kKcBlock), 0, s, nnz, A.colidx, (const int32_t*)row_of_edge, (const int32_t*)fslot,
                       (const int32_t*)rslot, (const int64_t*)rowptr, entries);
  GM_TRY_HIP(hipEventRecord(ev[1], s));

  // the flags land in the graph's pinned block (a run's own; runs on one graph follow each other): measured, a pass's read costs
  // 16.5 us that way against 26.6 us into pageable memory
  KcFlags h_own;
  KcFlags& h = g->pinned_flag ? *(KcFlags*)g->pinned_flag : h_own;
  memset(&h, 0, sizeof(h));
  const unsigned level_grid = kc_grid(n) < (unsigned)kKcLevelGrid ? kc_grid(n) : (unsigned)kKcLevelGrid;
  int cur = 0;
  for (int64_t level = 0; level <= (int64_t)n; level++) {  // a level with alive vertices takes at least one of them away
    const int slot = (int)(level & 1);
    hipLaunchKernelGGL(k_kc_level_min, dim3(level_grid), dim3(kKcBlock), 0, s, (const int32_t*)d_core, deg, n, flags, slot);
    hipLaunchKernelGGL(k_kc_level_list, dim3(kc_grid(n)), dim3(kKcBlock), 0, s, (const int32_t*)d_core, deg, n, list[cur], flags, slot, cur);
    GM_TRY_HIP(hipMemcpyAsync(&h, flags, sizeof(h), hipMemcpyDeviceToHost, s));
    GM_TRY_HIP(hipStreamSynchronize(s));
    if (h.alive[slot] == 0) break;
    st.spmv_launches++;
    const int k = (int)h.kmin[slot];
    uint32_t len = h.len[cur];
    while (len > 0) {  // every listed vertex dies here and enters no list again: at most n passes in the whole call
      hipLaunchKernelGGL(k_kc_pass, dim3(kc_grid((int64_t)len * kKcLanes)), dim3(kKcBlock), 0, s, (const int32_t*)list[cur], len, (const int64_t*)rowptr,
                         (const int32_t*)entries, deg, d_core, k, list[cur ^ 1], long_list, (uint32_t)long_cap, flags, cur, n);
      GM_TRY_HIP(hipMemcpyAsync(&h, flags, sizeof(h), hipMemcpyDeviceToHost, s));
      GM_TRY_HIP(hipStreamSynchronize(s));
      st.iterations++;
      if (h.nlong > 0) {
        const uint32_t nlong = h.nlong < (uint32_t)long_cap ? h.nlong : (uint32_t)long_cap;
        hipLaunchKernelGGL(k_kc_long, dim3(nlong, kKcLongBlocks), dim3(kKcBlock), 0, s, (const int32_t*)long_list, (const int64_t*)rowptr,
                           (const int32_t*)entries, deg, k, list[cur ^ 1], flags, cur, n);
        GM_TRY_HIP(hipMemcpyAsync(&h, flags, sizeof(h), hipMemcpyDeviceToHost, s));
        GM_TRY_HIP(hipStreamSynchronize(s));
      }
      cur ^= 1;
      len = h.len[cur];
    }
  }
  GM_TRY_HIP(hipEventRecord(ev[2], s));
  // (c) the finish: unused slots got their 0 in k_kc_init, and kmax came with the last read of the flags
  GM_TRY_HIP(hipEventRecord(ev[3], s));
  GM_TRY_HIP(hipEventSynchronize(ev[3]));
  GM_TRY_HIP(hipGetLastError());
  if (h_kmax) *h_kmax = (int32_t)h.kmax;
  GM_TRY_HIP(hipEventElapsedTime(&st.send_ms, ev[0], ev[1]));
  GM_TRY_HIP(hipEventElapsedTime(&st.spmv_ms, ev[1], ev[2]));
  GM_TRY_HIP(hipEventElapsedTime(&st.apply_ms, ev[2], ev[3]));
  st.total_ms = st.send_ms + st.spmv_ms + st.apply_ms;
  for (hipEvent_t& e : ev) (void)hipEventDestroy(e);
  g->stats = st;
  return GM_OK;
}

}  // namespace gm

extern "C" int gm_run_kcore(gm_graph_t* g, int32_t* d_core, int32_t* h_kmax, gm_stream_t stream) {
  // argument errors first: nothing on the GPU is touched
  if (!g || !d_core) { gm::set_error("gm_run_kcore: null graph or output array"); return GM_ERR_INVALID; }
  const gm_graph_desc_t& d = g->desc;
  if (d.row_lo != 0 || d.row_hi != d.ndevice || d.nshards > 1 || g->xfn != nullptr) {
    gm::set_error("gm_run_kcore: whole graphs only (no shards, no row ranges)");
    return GM_ERR_UNSUPPORTED;
  }
  if (!g->out.present && !g->in.present) { gm::set_error("gm_run_kcore: the graph holds no adjacency"); return GM_ERR_UNSUPPORTED; }
  return gm::run_kcore(g, d_core, h_kmax, (hipStream_t)stream);
}
