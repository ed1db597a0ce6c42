// gm_graph.hip -- device-side construction of the adjacency (CSR by destination
// and CSR by source), replacing the reference's host pipeline
//   Graph::ReadEdgelist -> SpMat ctor (edge shuffle) -> DCSCTile ctor
//   (partition, __gnu_parallel::sort, column compaction) -> Transpose
// (include/Graph.h:210-246, include/GMDP/matrices/DCSCTile.h:241-381,
//  include/GMDP/matrices/SpMat.h:422-443).
//
// What must be preserved from the reference is the ORDER in which a row's
// messages are reduced: ascending native column id, duplicates adjacent
// (DCSCTile.h:41-58 sort key).  A stable 64-bit radix sort on (row << 32 | col)
// gives exactly that; everything else (row partitions per OpenMP thread, column
// compaction) is CPU-cache machinery that has no analogue here.
//
// This unit: the key sort, the CSR with its row classes (finish_csr), the degree-ranked device order, the graph's
// lifetime and the C-ABI.  The layouts built on top of the CSR live in gm_graph_tiles.hip, gm_graph_sweep.hip and
// gm_graph_blocked.hip; gm_build.hpp holds what the four units share.
#include <string.h>
#include <cstring>

#include <algorithm>
#include <cmath>
#include <vector>

#include "gm_build.hpp"

namespace gm {

// the layout options (declared in gm_build.hpp; g_blocked_rows: gm_graph_blocked.hip)
int g_short_row = GM_SHORT_ROW;   // tunable through gm_set_option (experiments); defaults are the documented ones
int g_giant_row = 0;  // 0 = choose per graph (see pick_giant_threshold)
int g_rank_cap = 0;   // experiment: > 0 ranks only vertices of total degree >= cap; the others keep native order behind them
int g_rank_by = 0;    // experiment: 0 rank vertices by total degree, 1 by out-degree, 2 by in-degree
int g_tile_min_row = GM_TILE_MIN_ROW;  // rows of more than this many edges are tiled
int g_tile_balance = 1;  // column tiles serve equally many gathers (1) or hold equally many vertices with edges (0)
int g_long_mid = 0;  // > 0: experiment -- wave rows of more than this many edges get a wave each (0 = GM_LONG_MID rule)
int g_sweep_slices = 1;  // 1: cut the device order into ntiles * k <= 64 slices and build the row-stationary sweep of the medium rows (gm_graph_sweep)
int g_sort_tile_lists = 1;  // column tiles: the wave-row lists by descending piece length (sort_rows_by_length)
int g_sweep_border_factor = 4;  // the medium / long border is lowered while it exceeds this many times a wave's share of a block per slice
// cost of a stream row in the waves' shares of a block, percent of a medium row's.  A stream row is gathered like a medium row AND its products are stored, and a
// slice ends at a workgroup barrier: with the rows counted alike (100) the waves that hold the stream groups -- the block's last -- were what every slice waited
// for.  RMAT-26, ms per iteration at 100 / 150 / 200 / 250 / 300 / 350 / 400 / 500 / 700: 3.555 / 3.412 / 3.312 / 3.299 / 3.277 / 3.318 / 3.335 / 3.425 / 3.662;
// RMAT-27 at 100 / 200 / 300 / 500: 7.63 / 7.38 / 7.34 / 7.87; RMAT-25 at 100 / 300 / 500: 1.89 / 1.76 / 1.89 (gm_set_option("sweep_stream_weight"))
int g_sweep_stream_weight = 300;
int g_sweep_stream = 1;  // the short rows ride the sweep as stream groups (gm_sweep_t.nstream; round 6, last session); 0: none built
int g_sweep_waves = 16;  // waves per workgroup the sweep's blocks are dealt over (16; 12: a 768-thread sweep that leaves room on every CU for the short rows' kernel beside it -- experiment of round 6)
int g_sweep_fold_share = 50;  // share (percent of an equal share) of a block's groups that the waves folding the long rows get
int g_sweep_long_row = 0;  // the sweep's medium / long border (edges per row): 0 = chosen per graph (build_sweep)
int g_sweep_acc_limit = GM_SWEEP_ACC_ROWS, g_sweep_long_limit = GM_SWEEP_LONG_SLOTS;  // rows per workgroup and launch of the sweep (tests force several launches with small values)
int g_own_wave_row = 4096;  // column tiles: rows of more than this many edges (whole graph) keep the wave / giant kernels in every tile (0: classes per tile piece)
int g_col_tiles = 0;  // default number of column tiles for graphs whose descriptor says 0 (0 = environment GRAPHMAT_COL_TILES, else none)


// edge ids outside [lo, hi] (the reference only asserts this in __DEBUG builds, edgelist.h; here an
// out-of-range id would index device arrays out of bounds, so it is checked before anything else)
__global__ void __launch_bounds__(kT)
k_validate_ids(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, int64_t nnz, int lo, int hi,
               unsigned long long* __restrict__ bad /* [0] count, [1] first offending edge + 1 */) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  bool b = false;
  if (e < nnz) {
    const int s = src[e], d = dst[e];
    b = s < lo || s > hi || d < lo || d > hi;
  }
  const unsigned long long m = __ballot(b);
  if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) {
    atomicAdd(&bad[0], (unsigned long long)__popcll(m));
    atomicMin(&bad[1], (unsigned long long)e + 1ull);
  }
}

// total degree (in + out) per native vertex, for the GM_LAYOUT_DEGREE ranking
__global__ void __launch_bounds__(kT)
k_degree(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, int64_t nnz, int nparts, int nv,
         int ids_are_native, uint32_t* __restrict__ deg, int rank_by) {
  int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= nnz) return;
  int s = src[e], d = dst[e];
  int sn = ids_are_native ? s : to_native0(s, nparts, nv);
  int dn = ids_are_native ? d : to_native0(d, nparts, nv);
  // total degree decides who is "live"; the ranking experiments weight one side
  atomicAdd(&deg[sn], rank_by == 1 ? 65537u : rank_by == 2 ? 1u : 1u);
  atomicAdd(&deg[dn], rank_by == 2 ? 65537u : 1u);
}

__global__ void __launch_bounds__(kT)
k_count_nonzero(const uint32_t* __restrict__ deg, int nv, unsigned long long* __restrict__ out) {
  int v = blockIdx.x * kT + threadIdx.x;
  unsigned long long m = __ballot(v < nv && deg[v] != 0u);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(out, (unsigned long long)__popcll(m));
}

// out[0] += the degrees of all vertices, out[1] += the degrees of the vertices above `thr` (how much of the graph sits on busy vertices)
__global__ void __launch_bounds__(kT)
k_degree_mass(const uint32_t* __restrict__ deg, int nv, uint32_t thr, unsigned long long* __restrict__ out) {
  unsigned long long all = 0, heavy = 0;
  for (int v = blockIdx.x * kT + threadIdx.x; v < nv; v += gridDim.x * kT) { const uint32_t d = deg[v]; all += d; if (d > thr) heavy += d; }
  for (int o = 32; o > 0; o >>= 1) { all += __shfl_down(all, o); heavy += __shfl_down(heavy, o); }
  if ((threadIdx.x & 63) == 0) { if (all) atomicAdd(&out[0], all); if (heavy) atomicAdd(&out[1], heavy); }
}

__global__ void __launch_bounds__(kT)
k_rank_keys(const uint32_t* __restrict__ deg, int nv, uint32_t* __restrict__ keys, int32_t* __restrict__ ids, uint32_t cap) {
  int v = blockIdx.x * kT + threadIdx.x;
  if (v >= nv) return;
  uint32_t d = deg[v];
  if (cap > 0 && d > 0 && d < cap) d = 1;
  keys[v] = 0xffffffffu - d;  // ascending sort => descending degree; stable => ties by native id
  ids[v] = v;
}

__global__ void __launch_bounds__(kT)
k_live_flags(const uint32_t* __restrict__ deg, int nv, uint32_t* __restrict__ live) {
  int v = blockIdx.x * kT + threadIdx.x;
  if (v < nv) live[v] = deg[v] ? 1u : 0u;
}
// how often every vertex is a column of the GM_DIR_OUT adjacency (= a source): the gathers its x entry will serve
__global__ void __launch_bounds__(kT)
k_col_weight(const int32_t* __restrict__ src, int64_t nnz, int nparts, int nv, int ids_are_native, uint32_t* __restrict__ w) {
  int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= nnz) return;
  const int s = src[e];
  atomicAdd(&w[ids_are_native ? s : to_native0(s, nparts, nv)], 1u);
}
// final weight of a vertex from its column count: count^p (p = pw100 / 100) plus c for every vertex with edges
__global__ void __launch_bounds__(kT)
k_tile_weight(const uint32_t* __restrict__ deg, const uint32_t* __restrict__ cnt, int nv, uint32_t c, int pw100, int by_vertices,
              unsigned long long* __restrict__ w) {
  int v = blockIdx.x * kT + threadIdx.x;
  if (v >= nv) return;
  unsigned long long x = 0;
  if (deg[v]) {
    if (by_vertices) x = 1;
    else if (pw100 == 100) x = (unsigned long long)cnt[v] + c;
    else x = (unsigned long long)(powf((float)cnt[v], (float)pw100 * 0.01f) + 0.5f) + c;
  }
  w[v] = x;
}
// tile of the k-th ranked vertex: tiles are contiguous NATIVE ranges that serve equally many gathers (weight_before =
// column occurrences of the vertices before it in native order, `total` of all); 255 = no edges
__global__ void __launch_bounds__(kT)
k_tile_of_ranked(const int32_t* __restrict__ order, int nv, const uint32_t* __restrict__ deg, const unsigned long long* __restrict__ weight_before,
                 unsigned long long total, int ntiles, uint8_t* __restrict__ tile) {
  int k = blockIdx.x * kT + threadIdx.x;
  if (k >= nv) return;
  const int v = order[k];
  unsigned long long t = total ? (unsigned long long)((double)weight_before[v] * (double)ntiles / (double)total) : 0ull;
  if (t >= (unsigned long long)ntiles) t = (unsigned long long)ntiles - 1ull;
  tile[k] = deg[v] ? (uint8_t)t : (uint8_t)255;
}

// rank k -> device id (k % nshards) * S + k / nshards
__global__ void __launch_bounds__(kT)
k_deal(const int32_t* __restrict__ order, int nv, int nshards, int S, int32_t* __restrict__ dev_of_native,
       int32_t* __restrict__ native_of_dev) {
  int k = blockIdx.x * kT + threadIdx.x;
  if (k >= nv) return;
  int v = order[k];
  int d = (k % nshards) * S + k / nshards;
  dev_of_native[v] = d;
  native_of_dev[d] = v;
}

// Sharded graphs with slices (graphmat_hip.h: gm_sweep_t.nsub): position k of the list sorted by (slice, degree rank) -- the j-th
// busiest vertex of slice t -- goes to owner (j + t) % G at position sb[t] + j / G of the owner's range (the rotation by t keeps
// the slices' busiest vertices from all landing on owner 0); vertices without edges (key 255) follow the live part of every range.
struct SliceDeal { int32_t hb[GM_MAX_SLICES + 2]; int32_t sb[GM_MAX_SLICES + 2]; };
__global__ void __launch_bounds__(kT)
k_deal_sliced(const int32_t* __restrict__ order, const uint8_t* __restrict__ key_sorted, int nv, int G, int S, int TS, SliceDeal sd,
              int32_t* __restrict__ dev_of_native, int32_t* __restrict__ native_of_dev) {
  const int k = blockIdx.x * kT + threadIdx.x;
  if (k >= nv) return;
  const int v = order[k];
  const int t = key_sorted[k] == 255 ? TS : (int)key_sorted[k];
  const int j = k - sd.hb[t];
  const int owner = t == TS ? j % G : (j + t) % G;
  const int d = owner * S + sd.sb[t] + j / G;
  dev_of_native[v] = d;
  native_of_dev[d] = v;
}

// key = (local device row, or nrows when the row is not in this shard) << 32 | NATIVE col:
// sorting by it stores a row's edges in the reference's reduction order.
__global__ void __launch_bounds__(kT)
k_make_keys(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, int64_t nnz, int by_dst, int nparts,
            int nv, int row_lo, int row_hi, int ids_are_native, const int32_t* __restrict__ dev_of_native,
            uint64_t* __restrict__ keys, uint32_t* __restrict__ idx, unsigned long long* __restrict__ kept) {
  // grid-stride, one atomic per workgroup at the end: with a workgroup (let alone a wave) per 256 edges the single
  // `kept` counter took 16.7 M same-address atomics at RMAT-26 -- 200 ms for a kernel that moves 20 GB
  unsigned int mine_count = 0;
  for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kT) {
    int s = src[e], d = dst[e];
    int sn = ids_are_native ? s : to_native0(s, nparts, nv);
    int dn = ids_are_native ? d : to_native0(d, nparts, nv);
    int rn = by_dst ? dn : sn;
    int c = by_dst ? sn : dn;
    int r = dev_of_native ? dev_of_native[rn] : rn;
    const bool mine = (r >= row_lo && r < row_hi);
    uint32_t rf = mine ? (uint32_t)(r - row_lo) : (uint32_t)(row_hi - row_lo);
    keys[e] = ((uint64_t)rf << 32) | (uint32_t)c;
    idx[e] = (uint32_t)e;
    mine_count += mine ? 1u : 0u;
  }
  __shared__ unsigned int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  for (int off = 32; off > 0; off >>= 1) mine_count += __shfl_down(mine_count, off, 64);
  if ((threadIdx.x & 63) == 0 && mine_count) atomicAdd(&s_cnt, mine_count);
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(kept, (unsigned long long)s_cnt);
}

__global__ void __launch_bounds__(kT)
k_unpack(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, int64_t n, const void* __restrict__ val,
         int val_bytes, const int32_t* __restrict__ dev_of_native, int32_t* __restrict__ colidx,
         void* __restrict__ vals) {
  int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (k >= n) return;
  int32_t cn = (int32_t)(uint32_t)keys[k];
  colidx[k] = dev_of_native ? dev_of_native[cn] : cn;
  if (vals) {
    uint32_t e = idx[k];
    if (val_bytes == 4) {
      ((uint32_t*)vals)[k] = ((const uint32_t*)val)[e];
    } else if (val_bytes == 8) {
      ((uint64_t*)vals)[k] = ((const uint64_t*)val)[e];
    } else {
      const unsigned char* s = (const unsigned char*)val + (size_t)e * val_bytes;
      unsigned char* d = (unsigned char*)vals + (size_t)k * val_bytes;
      for (int b = 0; b < val_bytes; b++) d[b] = s[b];
    }
  }
}

// rowptr[r] = first sorted position whose row field >= r  (r in [0, nrows])
__global__ void __launch_bounds__(kT)
k_rowptr(const uint64_t* __restrict__ keys, int64_t n, int nrows, int64_t* __restrict__ rowptr) {
  int r = blockIdx.x * kT + threadIdx.x;
  if (r > nrows) return;
  uint64_t target = (uint64_t)(uint32_t)r << 32;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < target) lo = mid + 1; else hi = mid;
  }
  rowptr[r] = lo;
}

// log2 histogram of the row lengths (bin b counts rows with 2^b <= edges < 2^(b+1))
__global__ void __launch_bounds__(kT)
k_deg_hist(const int64_t* __restrict__ rowptr, int nrows, unsigned int* __restrict__ hist) {
  __shared__ unsigned int sh[64];
  if (threadIdx.x < 64) sh[threadIdx.x] = 0;
  __syncthreads();
  int r = blockIdx.x * kT + threadIdx.x;
  if (r < nrows) {
    long long d = rowptr[r + 1] - rowptr[r];
    if (d > 0) atomicAdd(&sh[63 - __clzll(d)], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 64 && sh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], sh[threadIdx.x]);
}

// segment starts (runs of rows, see gm_csr_t) and row classes
__global__ void __launch_bounds__(kT)
// (own_wave != null, column tiles with row classes fixed per ROW: a flagged row is a one-wave-per-row or giant row in
// every tile, however short its piece, and no other row is -- gm_csr_t.rows_keep_stream)
k_row_flags(const int64_t* __restrict__ rowptr, int nrows, int short_row, int giant_row, const unsigned char* __restrict__ own_wave,
            unsigned char* __restrict__ start, unsigned char* __restrict__ ismid, unsigned char* __restrict__ isgiant) {
  int r = blockIdx.x * kT + threadIdx.x;
  if (r >= nrows) return;
  int64_t a = rowptr[r], b = rowptr[r + 1];
  const bool flagged = own_wave != nullptr && own_wave[r] && b > a;
  bool lng = (b - a) > short_row || flagged;
  bool st = (r == 0) || ((r & 255) == 0) || lng;
  if (!st) {
    int64_t pa = rowptr[r - 1];
    bool prev_long = (a - pa) > short_row || (own_wave != nullptr && own_wave[r - 1] && a > pa);
    st = prev_long || (a / GM_BLOCK_NNZ != pa / GM_BLOCK_NNZ);
  }
  const bool giant = (b - a) > giant_row && (own_wave == nullptr || flagged);
  start[r] = st ? 1 : 0;
  ismid[r] = (lng && !giant) ? 1 : 0;
  isgiant[r] = giant ? 1 : 0;
}

// edges per kernel class of the multiply: [0] row-blocks (rows of <= short_row edges), [1] 16-rows-per-wave rows,
// [2] one-wave-per-row rows (more than long_limit edges), [3] giant rows
__global__ void __launch_bounds__(kT)
k_class_edges(const int64_t* __restrict__ rowptr, int nrows, int short_row, int64_t long_limit, int giant_row,
              const unsigned char* __restrict__ own_wave, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_c[4];
  if (threadIdx.x < 4) s_c[threadIdx.x] = 0ull;
  __syncthreads();
  const int r = blockIdx.x * kT + threadIdx.x;
  if (r < nrows) {
    const int64_t len = rowptr[r + 1] - rowptr[r];
    if (len > 0) {
      int cls = len <= short_row ? 0 : len > giant_row ? 3 : len > long_limit ? 2 : 1;
      if (own_wave != nullptr) cls = own_wave[r] ? (len > giant_row ? 3 : 2) : (len <= short_row ? 0 : 1);
      atomicAdd(&s_c[cls], (unsigned long long)len);
    }
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_c[threadIdx.x]) atomicAdd(&out[threadIdx.x], s_c[threadIdx.x]);
}


// presence bits of the non-empty rows (bit r&31 of word r>>5)
__global__ void __launch_bounds__(kT)
k_rowbits(const int64_t* __restrict__ rowptr, int nrows, uint32_t* __restrict__ bits) {
  int r = blockIdx.x * kT + threadIdx.x;
  bool ne = r < nrows && rowptr[r + 1] > rowptr[r];
  unsigned long long m = __ballot(ne);
  if ((threadIdx.x & 63) == 0 && r < nrows) {
    bits[r >> 5] = (uint32_t)m;
    if (r + 32 < nrows) bits[(r >> 5) + 1] = (uint32_t)(m >> 32);
  }
}

// one past the last entry of the wave-row list whose row has more than `limit` edges
__global__ void __launch_bounds__(kT)
k_last_long(const int32_t* __restrict__ mid_row, int nmid, const int64_t* __restrict__ rowptr, int64_t limit, int* __restrict__ out) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= nmid) return;
  const int r = mid_row[i];
  if (rowptr[r + 1] - rowptr[r] > limit) atomicMax(out, i + 1);
}

__global__ void __launch_bounds__(kT)
k_mid_long_flags(const int32_t* __restrict__ mid_row, int nmid, const int64_t* __restrict__ rowptr, int64_t limit, int64_t max_len,
                 const unsigned char* __restrict__ own_wave, unsigned char* __restrict__ is_long, unsigned char* __restrict__ is_rest) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= nmid) return;
  const int r = mid_row[i];
  const int64_t len = rowptr[r + 1] - rowptr[r];
  const bool keep = len <= max_len, lg = own_wave != nullptr ? own_wave[r] != 0 : len > limit;
  is_long[i] = (keep && lg) ? 1 : 0;
  is_rest[i] = (keep && !lg) ? 1 : 0;
}

__global__ void __launch_bounds__(kT)
k_giant_extent(const int32_t* __restrict__ giant_row, int ngiant, const int64_t* __restrict__ rowptr,
               int64_t* __restrict__ ext) {
  int i = blockIdx.x * kT + threadIdx.x;
  if (i >= ngiant) return;
  ext[2 * i] = rowptr[giant_row[i]];
  ext[2 * i + 1] = rowptr[giant_row[i] + 1];
}

// a segment is a row-block iff its first row is short and it holds at least one edge
__global__ void __launch_bounds__(kT)
k_seg_flags(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ seg_row, int nseg, int short_row,
            const unsigned char* __restrict__ own_wave, unsigned char* __restrict__ isblk) {
  int i = blockIdx.x * kT + threadIdx.x;
  if (i >= nseg) return;
  int r0 = seg_row[i], r1 = seg_row[i + 1];
  int64_t n = rowptr[r1] - rowptr[r0];
  bool longrow = (r1 - r0 == 1) && (n > short_row || (own_wave != nullptr && own_wave[r0]));
  isblk[i] = (!longrow && n > 0) ? 1 : 0;
}

// out = [entries of mid_row whose row has more than long_limit edges][the others], both in list order,
// keeping only rows of at most max_len edges; *n_long / *n_total = sizes
static int partition_mid(const int32_t* mid_row, int nmid, const int64_t* rowptr, int64_t long_limit, int64_t max_len,
                         int32_t* out, int* n_long, unsigned int* n_total, hipStream_t s, const unsigned char* own_wave = nullptr) {
  DevArray<unsigned char> fl, fs;
  DevArray<unsigned int> cnt;
  int rc;
  if ((rc = fl.alloc((size_t)nmid)) || (rc = fs.alloc((size_t)nmid)) || (rc = cnt.alloc(4))) return rc;
  GM_LAUNCH_1D(k_mid_long_flags, nmid, s, mid_row, nmid, rowptr, long_limit, max_len, own_wave, fl, fs);
  unsigned int nl = 0, ns = 0;
  RocTemp tmp;
  if ((rc = select(mid_row, fl, out, cnt, (size_t)nmid, s, &tmp)) || (rc = read_back(&nl, cnt.p, s))) return rc;
  if ((rc = select(mid_row, fs, out + nl, cnt + 1, (size_t)nmid, s, &tmp)) || (rc = read_back(&ns, cnt.p + 1, s))) return rc;
  *n_long = (int)nl;
  *n_total = nl + ns;
  return GM_OK;
}

__global__ void __launch_bounds__(kT)
k_row_lengths(const int32_t* __restrict__ list, int n, const int64_t* __restrict__ rowptr, uint32_t* __restrict__ len) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const int r = list[i];
  len[i] = (uint32_t)(rowptr[r + 1] - rowptr[r]);
}
// list[0, n) reordered by descending row length (stable: rows of equal length keep their order).  The persistent
// 16-rows-per-wave kernel deals consecutive 16-entry groups to its waves round robin and a group takes as many 64-edge
// steps as its LONGEST row: in row order a column tile's pieces of neighbouring rows differ widely (RMAT-26: 77 % of the
// 16 x 64 slots of a step hold an edge, and the waves of one launch finish between 190 and 330 us); sorted, the rows of a
// group are equally long and every wave gets the same number of steps.
static int sort_rows_by_length(int32_t* list, int n, const int64_t* rowptr, hipStream_t s) {
  if (n < 2) return GM_OK;
  DevArray<uint32_t> k_in, k_out;
  DevArray<int32_t> v_out;
  int rc;
  if ((rc = k_in.alloc((size_t)n)) || (rc = k_out.alloc((size_t)n)) || (rc = v_out.alloc((size_t)n))) return rc;
  GM_LAUNCH_1D(k_row_lengths, n, s, list, n, rowptr, k_in);
  if ((rc = radix_sort_pairs_desc(k_in.p, k_out.p, list, v_out.p, (size_t)n, 32, s))) return rc;
  GM_TRY_HIP(hipMemcpyAsync(list, v_out, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  GM_TRY_HIP(hipStreamSynchronize(s));
  return GM_OK;
}

// The edges of one direction as keys (local device row << 32 | native col) sorted into the reference's reduction order, with the
// input position of every sorted edge; *kept = edges whose row this shard holds (they come first)
static int sort_edge_keys(gm_graph* g, int by_dst, int64_t nnz, const int32_t* d_src, const int32_t* d_dst, hipStream_t s, DevArray<uint64_t>& keys_sorted,
                          DevArray<uint32_t>& idx_sorted, unsigned long long* kept) {
  const gm_graph_desc_t& D = g->desc;
  DevArray<uint64_t> keys_in;
  DevArray<uint32_t> idx_in;
  DevArray<unsigned long long> kept_d;
  int rc;
  if ((rc = keys_in.alloc((size_t)nnz)) || (rc = keys_sorted.alloc((size_t)nnz)) || (rc = idx_in.alloc((size_t)nnz)) || (rc = idx_sorted.alloc((size_t)nnz)) || (rc = kept_d.alloc(1))) return rc;
  GM_TRY_HIP(kept_d.fill(0, 1, s));
  if (nnz > 0) {
    hipLaunchKernelGGL(k_make_keys, dim3(grid_for(nnz) < 16384 ? grid_for(nnz) : 16384), dim3(kT), 0, s, d_src, d_dst, nnz, by_dst, D.nparts,
                       D.nvertices, D.row_lo, D.row_hi, D.ids_are_native, g->dev_of_native, keys_in, idx_in, kept_d);
    GM_TRY_HIP(hipGetLastError());
    if ((rc = radix_sort_pairs(keys_in.p, keys_sorted.p, idx_in.p, idx_sorted.p, (size_t)nnz, 32u + (unsigned)bits_for((uint32_t)(D.row_hi - D.row_lo)), s))) return rc;
  }
  return read_back(kept, kept_d.p, s);
}

// Sorts the edges of one direction into the reference's reduction order and builds its CSR
// (and, for GM_DIR_OUT of a tiled graph, the per-tile CSRs from the same sorted keys).
static int build_direction(gm_graph* g, int by_dst, int64_t nnz, const int32_t* d_src, const int32_t* d_dst,
                           const void* d_val, hipStream_t s, CsrOwned* out) {
  const gm_graph_desc_t& D = g->desc;
  DevArray<uint64_t> keys;
  DevArray<uint32_t> idx;
  unsigned long long kept = 0;
  int rc;
  if ((rc = sort_edge_keys(g, by_dst, nnz, d_src, d_dst, s, keys, idx, &kept))) return rc;
  const bool tiled = by_dst && g->ntiles > 1;
  if ((rc = finish_csr(g, keys, idx, kept, d_val, s, out, tiled ? g_tile_min_row : -1))) return rc;
  if (tiled) return build_tiles(g, keys, idx, kept, d_val, s, out);
  if (by_dst && D.nshards > 1 && g->nslices > 1 && g_sweep_slices != 0) {  // a shard's rows through the sweep (gm_sweep_t.nsub)
    keys.free(); idx.free();  // (the sweep's own sorts want the room)
    return build_sweep(g, out, s);
  }
  return GM_OK;
}


// ---- distributed build (gm_graph_desc_t.edges_local): this rank holds a part of the edge list ----------
// key = (row inside its owner's slice) << 32 | NATIVE col, owner = the shard whose slice holds the row
__global__ void __launch_bounds__(kT)
k_owner_keys(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, int64_t nnz, int by_dst, int nparts, int nv,
             int S, int ids_are_native, const int32_t* __restrict__ dev_of_native, uint64_t* __restrict__ keys,
             uint16_t* __restrict__ owner, uint32_t* __restrict__ pos) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= nnz) return;
  const int s = src[e], d = dst[e];
  const int sn = ids_are_native ? s : to_native0(s, nparts, nv);
  const int dn = ids_are_native ? d : to_native0(d, nparts, nv);
  const int r = dev_of_native[by_dst ? dn : sn];
  const int q = r / S;
  keys[e] = ((uint64_t)(uint32_t)(r - q * S) << 32) | (uint32_t)(by_dst ? sn : dn);
  owner[e] = (uint16_t)q;
  pos[e] = (uint32_t)e;
}
// bounds[q] = first position of the sorted owner list whose owner is >= q  (q in [0, n_owners])
__global__ void k_owner_bounds(const uint16_t* __restrict__ owner_sorted, int64_t n, int n_owners, int64_t* __restrict__ bounds) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q > n_owners) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int)owner_sorted[mid] < q) lo = mid + 1; else hi = mid;
  }
  bounds[q] = lo;
}
// the edges in bucket order (owner, then input position): keys and values ready to travel
__global__ void __launch_bounds__(kT)
k_bucket_gather(const uint64_t* __restrict__ keys, const void* __restrict__ val, int val_bytes, const uint32_t* __restrict__ pos,
                int64_t n, uint64_t* __restrict__ keys_b, void* __restrict__ val_b) {
  const int64_t j = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (j >= n) return;
  const uint32_t p = pos[j];
  keys_b[j] = keys[p];
  if (val_b) {
    if (val_bytes == 4) ((uint32_t*)val_b)[j] = ((const uint32_t*)val)[p];
    else if (val_bytes == 8) ((uint64_t*)val_b)[j] = ((const uint64_t*)val)[p];
    else {
      const unsigned char* a = (const unsigned char*)val + (size_t)p * val_bytes;
      unsigned char* b = (unsigned char*)val_b + (size_t)j * val_bytes;
      for (int i = 0; i < val_bytes; i++) b[i] = a[i];
    }
  }
}

// One direction from this rank's part of the edges: bucket them by the shard that owns their row, hand every
// shard its bucket (one padded all-gather per owner; a rank keeps what is addressed to it, in rank order, so
// duplicates of an edge stay in "rank, then input position" order), sort what arrived, build the CSR.
static int build_direction_local(gm_graph* g, int by_dst, int64_t nnz, const int32_t* d_src, const int32_t* d_dst,
                                 const void* d_val, hipStream_t s, CsrOwned* out) {
  const gm_graph_desc_t& D = g->desc;
  // (whether values travel is a property of the graph, not of this rank's part: a rank without edges may pass no array)
  const int N = D.nshards, me = D.shard, S = D.row_hi - D.row_lo, vb = D.val_bytes > 0 ? D.val_bytes : 0;
  const int64_t missing_vals = (vb && nnz > 0 && !d_val) ? 1 : 0;
  int rc;
  DevArray<uint64_t> keys;
  DevArray<uint32_t> pos_out;
  std::vector<int64_t> bounds((size_t)N + 1, 0);
  if (nnz > 0) {  // this rank's edges, bucketed by the shard that owns their row
    DevArray<uint16_t> owner_in, owner_out;
    DevArray<uint32_t> pos_in;
    DevArray<int64_t> bounds_d;
    if ((rc = keys.alloc((size_t)nnz)) || (rc = owner_in.alloc((size_t)nnz)) || (rc = owner_out.alloc((size_t)nnz)) || (rc = pos_in.alloc((size_t)nnz)) ||
        (rc = pos_out.alloc((size_t)nnz)) || (rc = bounds_d.alloc((size_t)N + 1)))
      return rc;
    GM_LAUNCH_1D(k_owner_keys, nnz, s, d_src, d_dst, nnz, by_dst, D.nparts, D.nvertices, S, D.ids_are_native, g->dev_of_native, keys, owner_in, pos_in);
    if ((rc = radix_sort_pairs(owner_in.p, owner_out.p, pos_in.p, pos_out.p, (size_t)nnz, (unsigned)std::max(1, bits_for((uint32_t)(N - 1))), s))) return rc;
    hipLaunchKernelGGL(k_owner_bounds, dim3((N + 1 + 63) / 64), dim3(64), 0, s, owner_out, nnz, N, bounds_d);
    if ((rc = read_back(bounds.data(), bounds_d.p, s, (size_t)N + 1))) return rc;
  }
  // cnt[p * N + q] = edges on rank p whose row shard q owns
  std::vector<int64_t> mine((size_t)N + 1), cnt((size_t)N * N), bytes((size_t)N);
  for (int q = 0; q < N; q++) mine[(size_t)q] = bounds[(size_t)q + 1] - bounds[(size_t)q];
  mine[(size_t)N] = missing_vals;
  {
    void* all = nullptr;
    if ((rc = gm_dist_allgatherv_host(mine.data(), (int64_t)(N + 1) * 8, &all, bytes.data())) != GM_OK) return rc;
    int64_t bad = 0;
    for (int p = 0; p < N; p++) {
      memcpy(&cnt[(size_t)p * N], (const int64_t*)all + (size_t)p * (N + 1), (size_t)N * 8);
      bad += ((const int64_t*)all)[(size_t)p * (N + 1) + N];
    }
    gm_host_free(all);
    if (bad) { set_error("gm_graph_create: val_bytes = %d but %lld rank(s) passed edges without values", vb, (long long)bad); return GM_ERR_INVALID; }
  }
  int64_t maxm = 0, kept = 0;
  for (int q = 0; q < N; q++)
    for (int p = 0; p < N; p++) maxm = std::max(maxm, cnt[(size_t)p * N + q]);
  for (int p = 0; p < N; p++) kept += cnt[(size_t)p * N + me];
  if (kept >= (1ll << 32)) { set_error("gm_graph_create: shard %d would hold more than 2^32-1 edges", me); return GM_ERR_UNSUPPORTED; }
  DevArray<uint64_t> rk_in;  // what arrived: keys and (rvals) values, in "rank, then input position" order
  DevBuf rvals;
  {
    // send buffers in bucket order, padded so that a full-size block can be read from every bucket start
    DevArray<uint64_t> send_k, gk;
    DevBuf send_v, gv;
    if ((rc = send_k.alloc((size_t)(nnz + maxm))) || (vb && (rc = send_v.alloc((size_t)(nnz + maxm) * vb)))) return rc;
    if (nnz > 0) GM_LAUNCH_1D(k_bucket_gather, nnz, s, keys, d_val, vb, pos_out, nnz, send_k, vb ? (void*)send_v.p : nullptr);
    GM_TRY_HIP(hipStreamSynchronize(s));
    keys.free(); pos_out.free();  // (room for what arrives)
    if ((rc = rk_in.alloc((size_t)kept)) || (rc = gk.alloc((size_t)N * maxm)) || (vb && ((rc = rvals.alloc((size_t)kept * vb)) || (rc = gv.alloc((size_t)N * maxm * vb))))) return rc;
    for (int q = 0; q < N; q++) {
      int64_t m = 0;
      for (int p = 0; p < N; p++) m = std::max(m, cnt[(size_t)p * N + q]);
      if (m == 0) continue;
      if ((rc = dist_all_gather_bytes(send_k + bounds[(size_t)q], gk, (size_t)m * 8, s))) return rc;
      if (vb && (rc = dist_all_gather_bytes(send_v + (size_t)bounds[(size_t)q] * vb, gv, (size_t)m * vb, s))) return rc;
      if (q == me) {
        int64_t off = 0;
        for (int p = 0; p < N; p++) {
          const int64_t c = cnt[(size_t)p * N + me];
          if (c > 0) {
            GM_TRY_HIP(hipMemcpyAsync(rk_in + off, gk + (size_t)p * m, (size_t)c * 8, hipMemcpyDeviceToDevice, s));
            if (vb) GM_TRY_HIP(hipMemcpyAsync(rvals + (size_t)off * vb, gv + (size_t)p * m * vb, (size_t)c * vb, hipMemcpyDeviceToDevice, s));
          }
          off += c;
        }
      }
      GM_TRY_HIP(hipStreamSynchronize(s));  // the gather buffers are reused by the next owner
    }
  }
  DevArray<uint64_t> rk_out;
  DevArray<uint32_t> ri_out;
  {
    DevArray<uint32_t> ri_in;
    if ((rc = rk_out.alloc((size_t)kept)) || (rc = ri_in.alloc((size_t)kept)) || (rc = ri_out.alloc((size_t)kept))) return rc;
    if (kept > 0) {
      GM_LAUNCH_1D(k_fill_iota<uint32_t>, kept, s, ri_in, kept);
      if ((rc = radix_sort_pairs(rk_in.p, rk_out.p, ri_in.p, ri_out.p, (size_t)kept, 32u + (unsigned)bits_for((uint32_t)S), s))) return rc;
    }
    GM_TRY_HIP(hipStreamSynchronize(s));
    rk_in.free();
  }
  if ((rc = finish_csr(g, rk_out, ri_out, (unsigned long long)kept, vb ? (const void*)rvals.p : nullptr, s, out, -1))) return rc;
  if (by_dst && N > 1 && g->nslices > 1 && g_sweep_slices != 0) {
    rk_out.free(); ri_out.free(); rvals.free();  // (the sweep's own sorts want the room)
    return build_sweep(g, out, s);
  }
  return GM_OK;
}


// Giant-row threshold.  The per-row workgroups of k_spmv_giant are the right tool for the few
// rows whose serial chain would otherwise dominate, and the wrong one for thousands of merely
// long rows, so the threshold is the smallest power of two >= 4096 that leaves at most 1024
// rows above it (GM_GIANT_ROW documents the typical outcome at RMAT-24..27).
static int pick_giant_threshold(const int64_t* rowptr, int nrows, hipStream_t s, int* giant_row) {
  DevArray<unsigned int> hist;
  int rc;
  if ((rc = hist.alloc(64))) return rc;
  GM_TRY_HIP(hist.fill(0, 64, s));
  if (nrows > 0) GM_LAUNCH_1D(k_deg_hist, nrows, s, rowptr, nrows, hist);
  unsigned int h[64];
  if ((rc = read_back(h, hist.p, s, 64))) return rc;
  int b = 40;
  unsigned long long above = 0;
  while (b > 12 && above + h[b - 1] <= 1024) { above += h[b - 1]; b--; }
  *giant_row = (b >= 31) ? 0x7fffffff : (1 << b);  // rows of >= 2^b edges (~ > giant_row) are giant
  return GM_OK;
}

// CSR arrays and work decomposition from `kept` sorted keys (row << 32 | native col) and, for the
// edge values, the input position of every sorted edge.
// tile_split >= 0 (whole-graph CSR of a tiled graph): also list the wave rows of at most tile_split edges.
// own_wave != null (a column tile): row classes fixed per row, see k_row_flags.
int finish_csr(gm_graph* g, const uint64_t* keys_sorted, const uint32_t* idx_sorted, unsigned long long kept,
               const void* d_val, hipStream_t s, CsrOwned* out, int tile_split, const unsigned char* own_wave) {
  const int short_row = g_short_row;
  const gm_graph_desc_t& D = g->desc;
  const int nrows = D.row_hi - D.row_lo;
  int rc;
  DevArray<int64_t> rowptr;
  DevArray<int32_t> colidx;
  DevBuf vals;
  if ((rc = rowptr.alloc((size_t)nrows + 1)) || (rc = colidx.alloc((size_t)kept))) return rc;
  const bool keep_vals = D.val_bytes > 0 && d_val != nullptr;
  if (keep_vals && (rc = vals.alloc((size_t)kept * D.val_bytes))) return rc;
  if (kept > 0)
    GM_LAUNCH_1D(k_unpack, kept, s, keys_sorted, idx_sorted, (int64_t)kept, d_val, D.val_bytes, g->dev_of_native, colidx, keep_vals ? (void*)vals.p : nullptr);
  GM_LAUNCH_1D(k_rowptr, nrows + 1, s, keys_sorted, (int64_t)kept, nrows, rowptr);
  GM_TRY_HIP(hipGetLastError());

  const size_t nbitwords = (size_t)(nrows + 31) / 32 + 2;
  DevArray<uint32_t> rbits;
  if ((rc = rbits.alloc(nbitwords))) return rc;
  GM_TRY_HIP(rbits.fill(0, nbitwords, s));
  if (nrows > 0) GM_LAUNCH_1D(k_rowbits, nrows, s, rowptr, nrows, rbits);

  int giant_row = g_giant_row;
  if (giant_row <= 0 && (rc = pick_giant_threshold(rowptr, nrows, s, &giant_row))) return rc;

  // work decomposition: segments, row-blocks, wave rows, giant rows
  DevArray<unsigned char> f0, f1, f2;
  DevArray<int32_t> seg, blkl, mid, giant;
  DevArray<unsigned int> cnt;
  if ((rc = f0.alloc((size_t)nrows + 1)) || (rc = f1.alloc((size_t)nrows + 1)) || (rc = f2.alloc((size_t)nrows + 1)) || (rc = seg.alloc((size_t)nrows + 2)) ||
      (rc = mid.alloc((size_t)nrows + 1)) || (rc = giant.alloc((size_t)nrows + 1)) || (rc = cnt.alloc(8)))
    return rc;
  unsigned int nseg = 0, nblk = 0, nmid = 0, ngiant = 0;
  if (nrows > 0) {
    GM_LAUNCH_1D(k_row_flags, nrows, s, rowptr, nrows, short_row, giant_row, own_wave, f0, f1, f2);
    GM_TRY_HIP(hipGetLastError());
    rocprim::counting_iterator<int32_t> ids(0);
    unsigned int h[3] = {0, 0, 0};
    RocTemp tmp;  // (the three lists are queued back to back)
    if ((rc = select(ids, f0, seg.p, cnt, (size_t)nrows, s, &tmp)) || (rc = select(ids, f1, mid.p, cnt + 1, (size_t)nrows, s, &tmp)) ||
        (rc = select(ids, f2, giant.p, cnt + 2, (size_t)nrows, s, &tmp)) || (rc = read_back(h, cnt.p, s, 3)))
      return rc;
    nseg = h[0];
    nmid = h[1];
    ngiant = h[2];
    int32_t last = nrows;
    GM_TRY_HIP(hipMemcpyAsync(seg + nseg, &last, 4, hipMemcpyHostToDevice, s));
    // row-blocks = the segments that hold short rows with at least one edge
    if ((rc = blkl.alloc((size_t)nseg + 1))) return rc;
    GM_LAUNCH_1D(k_seg_flags, nseg, s, rowptr, seg, (int)nseg, short_row, own_wave, f0);
    if ((rc = select(ids, f0, blkl.p, cnt + 3, (size_t)nseg, s, &tmp)) || (rc = read_back(&nblk, cnt.p + 3, s))) return rc;
  } else {
    if ((rc = blkl.alloc(4))) return rc;
  }

  // wave rows: where the long ones (more than GM_LONG_MID edges) end in the list
  // (with a million wave rows there are plenty of 16-row groups to keep the chip busy, and rows of up to
  // 4096 edges can be grouped too: RMAT-26 8.02 -> 7.87 ms; on RMAT-22 that limit costs 17 %)
  const int64_t long_limit = g_long_mid > 0 ? (int64_t)g_long_mid : nmid >= (1u << 20) ? 4 * (int64_t)GM_LONG_MID : (int64_t)GM_LONG_MID;
  int nmid_long = 0, numid_long = 0;
  unsigned int numid = 0;
  DevArray<int32_t> umid;
  if (nmid > 0) {
    GM_TRY_HIP(cnt.fill(0, 1, s));
    if (g->ntiles > 1) {
      // tiled device order = (tile, degree rank): the long rows are no prefix of the row-ordered list,
      // so the list is partitioned instead: [long rows][the rest], each part in row order
      DevArray<int32_t> mid2;
      if ((rc = mid2.alloc((size_t)nrows + 1))) return rc;
      unsigned int n_all = 0;
      if ((rc = partition_mid(mid, (int)nmid, rowptr, long_limit, (int64_t)1 << 62, mid2, &nmid_long, &n_all, s, own_wave))) return rc;
      if (tile_split >= 0) {  // the wave rows that stay untiled, same layout
        if ((rc = umid.alloc((size_t)nmid + 1))) return rc;
        if ((rc = partition_mid(mid, (int)nmid, rowptr, long_limit, (int64_t)tile_split, umid, &numid_long, &numid, s))) return rc;
      }
      // a column tile's lists by descending piece length (gm_set_option("sort_tile_lists", 0): row order, for A/B runs)
      if (own_wave != nullptr && g_sort_tile_lists != 0) {
        if ((rc = sort_rows_by_length(mid2, nmid_long, rowptr, s))) return rc;
        if ((rc = sort_rows_by_length(mid2 + nmid_long, (int)n_all - nmid_long, rowptr, s))) return rc;
      }
      mid = std::move(mid2);
    } else {
      GM_LAUNCH_1D(k_last_long, nmid, s, mid, (int)nmid, rowptr, long_limit, (int*)cnt.p);
      if ((rc = read_back(&nmid_long, (const int*)cnt.p, s))) return rc;
    }
  }

  // edges per kernel class (reporting: the per-kernel edge rates of bench.py)
  unsigned long long h_class[4] = {0, 0, 0, 0};
  {
    DevArray<unsigned long long> cls;
    if ((rc = cls.alloc(4))) return rc;
    GM_TRY_HIP(cls.fill(0, 4, s));
    if (nrows > 0) GM_LAUNCH_1D(k_class_edges, nrows, s, rowptr, nrows, short_row, long_limit, giant_row, own_wave, cls);
    if ((rc = read_back(h_class, cls.p, s, 4))) return rc;
  }

  // pieces of the giant rows for the parallel products pass
  DevArray<int32_t> gcr;
  DevArray<int64_t> gce, gto;
  std::vector<int32_t> h_gcr;
  std::vector<int64_t> h_gce, h_gto(1, 0);
  if (ngiant > 0) {
    DevArray<int64_t> ext;
    if ((rc = ext.alloc((size_t)ngiant * 2))) return rc;
    GM_LAUNCH_1D(k_giant_extent, ngiant, s, giant, (int)ngiant, rowptr, ext);
    std::vector<int64_t> h_ext((size_t)ngiant * 2);
    if ((rc = read_back(h_ext.data(), ext.p, s, (size_t)ngiant * 2))) return rc;
    for (unsigned i = 0; i < ngiant; i++) {
      for (int64_t e = h_ext[2 * i]; e < h_ext[2 * i + 1]; e += GM_GIANT_CHUNK) {
        h_gcr.push_back((int32_t)i);
        h_gce.push_back(e);
      }
      h_gto.push_back(h_gto.back() + ((h_ext[2 * i + 1] - h_ext[2 * i]) + 63) / 64 * 64);
    }
  }
  if ((rc = gcr.alloc(h_gcr.size())) || (rc = gce.alloc(h_gce.size())) || (rc = gto.alloc(h_gto.size()))) return rc;
  if (!h_gcr.empty()) {
    GM_TRY_HIP(hipMemcpyAsync(gcr, h_gcr.data(), h_gcr.size() * 4, hipMemcpyHostToDevice, s));
    GM_TRY_HIP(hipMemcpyAsync(gce, h_gce.data(), h_gce.size() * 8, hipMemcpyHostToDevice, s));
  }
  GM_TRY_HIP(hipMemcpyAsync(gto, h_gto.data(), h_gto.size() * 8, hipMemcpyHostToDevice, s));
  DevBuf gst;  // 32-byte records of the giant-row kernels, one per 512-product sub-piece = 8 per piece (kernels.hpp: gchunk_state; no hints yet)
  const size_t gst_bytes = h_gcr.size() * (GM_GIANT_CHUNK / 512) * 32 + 64;  // (32-byte records: a hint and the maps of three binades)
  if ((rc = gst.alloc(gst_bytes))) return rc;
  GM_TRY_HIP(gst.fill(0, gst_bytes, s));
  GM_TRY_HIP(hipStreamSynchronize(s));

  out->rowptr = rowptr.release();
  out->colidx = colidx.release();
  out->vals = keep_vals ? vals.release() : nullptr;
  out->rowbits = rbits.release();
  out->seg_row = seg.release();
  out->blk_seg = blkl.release();
  out->mid_row = mid.release();
  out->giant_row = giant.release();
  out->gchunk_row = gcr.release();
  out->gchunk_edge = gce.release();
  out->gterm_off = gto.release();
  out->umid_row = numid > 0 ? umid.release() : nullptr;
  out->gchunk_state = gst.release();
  out->present = true;
  gm_csr_t& v = out->view;
  v.nnz = (int64_t)kept;
  v.nrows = nrows;
  v.row_base = D.row_lo;
  v.ncols = D.ndevice;
  v.val_bytes = keep_vals ? D.val_bytes : 0;
  v.rowptr = out->rowptr;
  v.colidx = out->colidx;
  v.vals = out->vals;
  v.rowbits = out->rowbits;
  v.seg_row = out->seg_row;
  v.nseg = (int32_t)nseg;
  v.blk_seg = out->blk_seg;
  v.nblk = (int32_t)nblk;
  v.mid_row = out->mid_row;
  v.nmid = (int32_t)nmid;
  v.giant_row = out->giant_row;
  v.ngiant = (int32_t)ngiant;
  v.gchunk_row = out->gchunk_row;
  v.gchunk_edge = out->gchunk_edge;
  v.gterm_off = out->gterm_off;
  v.ngchunk = (int32_t)h_gcr.size();
  v.giant_edges = h_gto.back();
  v.short_row = short_row;
  v.nmid_long = nmid_long;
  v.umid_row = out->umid_row;
  v.numid = (int32_t)numid;
  v.numid_long = numid_long;
  v.tile_min_row = tile_split;
  v.gchunk_state = out->gchunk_state;
  v.edges_blk = (int64_t)h_class[0];
  v.edges_wave16 = (int64_t)h_class[1];
  v.edges_wave = (int64_t)h_class[2];
  v.rows_keep_stream = own_wave != nullptr ? 1 : 0;
  v.cold_from = 0;
  v.hot_base = 0;
  v.hot_len = D.ndevice;
  v.hot_slices = 1;
  v.hot_stride = 0;
  if (D.layout == GM_LAYOUT_DEGREE && D.nshards > 1) {  // rank k lives in slice k % G at position k / G
    v.hot_slices = D.nshards;
    v.hot_stride = D.ndevice / D.nshards;
    v.hot_len = v.hot_stride;
  }
  return GM_OK;
}

// edge values rewritten in the CSR: the sweep's copies follow (gm_graph_sync_tile_vals)
__global__ void __launch_bounds__(kT)
k_sweep_sync_vals(const uint32_t* __restrict__ src_pos, size_t n, const uint32_t* __restrict__ vals, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kT + threadIdx.x;
  if (i < n && src_pos[i] != 0xffffffffu) out[i] = vals[src_pos[i]];
}
// GM_LAYOUT_DEGREE: rank vertices by total degree, deal the ranks round-robin over the shards
static int build_degree_layout(gm_graph* g, int64_t nnz, const int32_t* d_src, const int32_t* d_dst, hipStream_t s, bool keeps_values) {
  gm_graph_desc_t& D = g->desc;
  const int nv = D.nvertices, G = D.nshards;
  int S = (nv + G - 1) / G;
  if (G > 1) S = (S + 63) / 64 * 64;
  int vd = (G > 1) ? G * S : nv;  // (sharded graphs with slices: S and vd are settled once the slices are known, below)
  DevArray<uint32_t> deg, keys_in, keys_out;
  DevArray<int32_t> ids_in, order, don, nod;
  int rc;
  if ((rc = deg.alloc((size_t)nv)) || (rc = keys_in.alloc((size_t)nv)) || (rc = keys_out.alloc((size_t)nv)) || (rc = ids_in.alloc((size_t)nv)) || (rc = order.alloc((size_t)nv)) ||
      (rc = don.alloc((size_t)nv)))
    return rc;
  GM_TRY_HIP(deg.fill(0, (size_t)nv, s));
  if (nnz > 0) GM_LAUNCH_1D(k_degree, nnz, s, d_src, d_dst, nnz, D.nparts, nv, D.ids_are_native, deg, g_rank_by);
  if (D.edges_local && (rc = dist_all_reduce_sum_u32(deg, (size_t)nv, s))) return rc;  // counts of all parts
  GM_LAUNCH_1D(k_rank_keys, nv, s, deg, nv, keys_in, ids_in, (uint32_t)(g_rank_by == 0 ? g_rank_cap : 0));
  if ((rc = radix_sort_pairs(keys_in.p, keys_out.p, ids_in.p, order.p, (size_t)nv, 32, s))) return rc;
  // vertices with at least one edge come first in every slice: the rest is never gathered
  DevArray<unsigned long long> nzd;
  if ((rc = nzd.alloc(1))) return rc;
  GM_TRY_HIP(nzd.fill(0, 1, s));
  GM_LAUNCH_1D(k_count_nonzero, nv, s, deg, nv, nzd);
  unsigned long long nz = 0;
  if ((rc = read_back(&nz, nzd.p, s))) return rc;
  g->nlive = (int32_t)nz;
  // column tiles: contiguous NATIVE ranges; the device order becomes (tile, degree rank inside the tile),
  // vertices without edges last.  A stable sort of the ranked list by tile does it.
  int T = D.col_tiles;
  const double mib_live = (double)nz * 4.0 / 1048576.0;
  if (T == 0) T = g_col_tiles;
  if (T == 0) { const char* e = getenv("GRAPHMAT_COL_TILES"); if (e) T = atoi(e); }
  if (T == 0) {
    // automatic: tiles pay once the live part of a 4-byte message vector outgrows what the caches hold.  Measured,
    // PageRank on RMAT with tiles that serve equally many gathers and row classes fixed per row (g_own_wave_row; ms per
    // iteration by tile count): RMAT-24 (34 MiB live) 1 / 3 / 4: 1.67 / 1.85 / 1.84; RMAT-25 (65 MiB) 4 / 5 / 6 / 7: 3.41 /
    // 3.38 / 3.39 / 3.46; RMAT-26 (125 MiB) 5 / 6 / 7 / 8 / 9 / 10 / 12: 6.31 / 6.18 / 6.24 / 6.09-6.13 / 6.14 / 6.09 / 6.21;
    // RMAT-27 (239 MiB) 10 / 12 / 14 / 16: 13.24 / 13.24 / 12.99 / 13.03; RMAT-25 with the persistent kernels 4 / 5 / 6 / 7 / 8:
    // 3.18 / 3.10 / 3.15 / 3.31 / 3.31 -- about one tile per 17 MiB on top of one, from 60 MiB on
    // (with the auxiliary stream joined after every tile the optimum was fewer, larger tiles: 4 / 6 / 10)
    const double mib = (double)nz * 4.0 / 1048576.0;
    T = mib >= 60.0 ? (int)(1.0 + mib / 17.0 + 0.5) : 1;
    // With the row-stationary sweep (g_sweep_slices != 0; the closing session of round 4, profiles/r04_tile_counts_with_sweep.md) the
    // tiles only cut the one-wave-per-row and giant rows -- the medium rows walk ~64 slices whatever the tile count -- and every tile
    // is a pass of two latency-bound kernel chains: FEWER tiles win, and tiling pays from smaller graphs on because it brings the
    // sweep with it.  ms per iteration by tile count: RMAT-23 (18 MiB) 1 / 2 / 3: 0.820 / 0.842 / 0.857; RMAT-24 (34 MiB) 1 / 2 / 3:
    // 1.66 / 1.33 / 1.45; RMAT-25 (65 MiB) 2 / 3 / 4 / 5 / 6: 2.61 / 2.47 / 2.54 / 2.56 / 2.60; RMAT-26 (125 MiB) 2 .. 9: 5.26 / 4.84 / 4.92 /
    // 4.99 / 5.00 / 5.09 / 5.10 / 5.12 (seeds 2 and 3: 3 tiles best as well, 4.83 / 4.81); RMAT-27 (239 MiB) 3 / 4 / 5 / 6 / 8 / 10 / 12 / 15:
    // 11.84 / 11.20 / 11.27 / 11.15 / 11.14 / 11.30 / 11.38 / 11.49 -- two tiles from 25 MiB, three from 50 MiB, one per 40 MiB from 180 MiB on
    // (An adjacency that keeps its edge values is not swept -- the sweep's copy of the medium rows holds column ids only -- and all
    // its rows above 64 edges go through the tiles as before: the old rule stays for it, from 100 MiB on.  The reference's unchanged
    // PageRank.cpp -- int edge values, ordered fold -- by tile count: RMAT-24 1 / 2 / 3 / 5: 149 / 161 / 162 / 165 ms; RMAT-25 1 / 2 / 3 / 5:
    // 228 / 308 / 283 / 281 ms; RMAT-26 1 / 3 / 8: 641 / 582 / 506 ms.)
    // (round 5: the sweep -- kernels.hpp: k_spmv_sell -- also takes the rows of more than own_wave_row edges and adjacencies that keep
    // 4-byte edge values; the tiles are only walked by programs the sweep does not cover, and get the same count)
    // (round 6: with the giant rows' passes down to a third -- they were what the small graphs' iterations waited for -- the sweep pays from ~7 MiB on:
    // RMAT-22 (9 MiB) 0.445 -> 0.384 ms, RMAT-23 (18 MiB) 0.813 -> 0.589 ms with 2 x 8 slices; RMAT-21 (5 MiB) 0.295 -> 0.321, RMAT-20 0.207 -> 0.307:
    // profiles/r06_small_scales_sweep.txt.  The [slice][degree rank] order the sweep needs spreads the hub columns over the slices, which the
    // gather kernels of the programs that do NOT take the sweep pay for: unchanged SSSP.cpp RMAT-22 6.4 -> 7.8 ms, RMAT-23 11.4 -> 13.4 ms,
    // BFS.cpp +3..5 %, against PageRank.cpp 24.3 -> 24.8 ms (RMAT-22) and 52.3 -> 44.4 ms (RMAT-23) -- so the rule starts at 12 MiB, where PageRank
    // gains 28 %, not at 7.  Shards keep the 25 MiB rule: nothing smaller was measured on them.)
    const double sweep_from = G > 1 ? 25.0 : 12.0;
    if (g_sweep_slices != 0 && (!keeps_values || D.val_bytes == 4)) T = mib < sweep_from ? 1 : mib < 50.0 ? 2 : mib < 180.0 ? 3 : (int)(mib / 40.0 + 0.5);
    else if (keeps_values && mib < 100.0) T = 1;
  }
  // Sharded graphs (round 6): no column tiles, but the same SLICES -- every owner's range of the device order becomes [slice][degree rank
  // inside it], so that a slice of the message vector is the same sub-range of all G owners' ranges and the row-stationary sweep can walk
  // a shard's rows (gm_sweep_t.nsub).  Whenever a single-shard graph of this size would be tiled (or the caller asks for tiles).
  const bool sweepable_ = !keeps_values || D.val_bytes == 4;
  const bool shard_slices = G > 1 && T > 1 && nz >= 2 && g_sweep_slices != 0 && sweepable_ && nnz >= 0 && nv < (1 << 28);
  if (T < 1 || G > 1 || nz < 2) T = 1;
  if (T > GM_MAX_TILES) T = GM_MAX_TILES;
  DevArray<uint8_t> slice_keys;  // sharded graphs with slices: the slice of every position of the sorted list (255 = no edges)
  SliceDeal sd;
  memset(&sd, 0, sizeof(sd));
  int shard_TS = 0;
  if (T > 1 || shard_slices) {
    // Tiles are contiguous NATIVE ranges cut so that every tile serves about the same number of gathers (a vertex weighs
    // as often as it is a column of the GM_DIR_OUT adjacency; on RMAT the busy tiles then hold fewer vertices, i.e. a
    // smaller slice of x where most gathers go).  gm_set_option("tile_balance", 0) cuts them into equally many vertices
    // with edges instead: RMAT-26 best 4 such tiles 7.07 ms against 6.74 ms with 6 gather-balanced ones.
    DevArray<uint32_t> cnt;
    DevArray<unsigned long long> w, wpre;
    DevArray<uint8_t> tk_in, tk_out;
    DevArray<int32_t> order2;
    DevArray<int64_t> bnd;
    if ((rc = cnt.alloc((size_t)nv)) || (rc = w.alloc((size_t)nv + 1)) || (rc = wpre.alloc((size_t)nv + 1)) || (rc = tk_in.alloc((size_t)nv)) || (rc = tk_out.alloc((size_t)nv)) ||
        (rc = order2.alloc((size_t)nv)) || (rc = bnd.alloc((size_t)GM_MAX_SLICES + 2)))
      return rc;
    GM_TRY_HIP(cnt.fill(0, (size_t)nv, s));
    GM_TRY_HIP(w.fill(0, (size_t)nv + 1, s));
    // g_tile_balance: 0 = vertices; 1 = gathers; 2..65536 = gathers + (value - 1) per vertex; 100000 + X = gathers^(X/100)  (experiments)
    const int by_vertices = (g_tile_balance == 0 || nnz == 0) ? 1 : 0;
    const int pw100 = g_tile_balance >= 100000 ? g_tile_balance - 100000 : 100;
    const uint32_t addc = (g_tile_balance >= 2 && g_tile_balance <= 65536) ? (uint32_t)(g_tile_balance - 1) : 0u;
    if (!by_vertices && nnz > 0) GM_LAUNCH_1D(k_col_weight, nnz, s, d_src, nnz, D.nparts, nv, D.ids_are_native, cnt);
    if (!by_vertices && D.edges_local && (rc = dist_all_reduce_sum_u32(cnt, (size_t)nv, s))) return rc;  // (every rank must cut the same slices)
    GM_LAUNCH_1D(k_tile_weight, nv, s, deg, cnt, nv, addc, pw100, by_vertices, w);
    unsigned long long total = 0;
    if ((rc = exclusive_scan(w.p, wpre.p, (size_t)nv + 1, s)) || (rc = read_back(&total, wpre.p + nv, s))) return rc;
    // (gm_graph_sweep: the order is cut k times finer than the tiles, a tile = k consecutive slices; about 1.3 MiB of live
    // messages per slice -- measured with the sweep's prototype, tools/sell_bench.hip: RMAT-26 (125 MiB) 64 / 80 / 96 / 128 slices
    // 2.17 / 2.09 / 2.05 / 2.15 ms for the swept rows, RMAT-25 (65 MiB) 32 / 64: 1.02 / 0.94 ms, RMAT-24 (34 MiB) 16 / 32 / 64: 0.79 / 0.80 / 0.92)
    // (a graph WITHOUT skew -- next to no edge on a vertex of more than 2 x short_row edges: the shape of the reference's test/generator.h --
    // is multiplied by the column-blocked stream of its short rows, k_spmv_blocked, whose synchronised steps want fewer, larger slices:
    // uniform 2^26, 32 / 48 / 56 / 64 / 72 / 96 / 128 slices: 12.9 / 10.5 / 9.7 / 9.0 / 10.0 / 10.1 / 12.0 ms; 2^25, 32 / 99: 4.24 / 4.71 -- about 4 MiB each)
    bool no_skew = false;
    if (g_sweep_slices == 1 && g_blocked_rows >= 0 && !keeps_values && nnz > 0 && G == 1) {
      DevArray<unsigned long long> mass;
      if ((rc = mass.alloc(2))) return rc;
      GM_TRY_HIP(mass.fill(0, 2, s));
      hipLaunchKernelGGL(k_degree_mass, dim3(1024), dim3(kT), 0, s, deg, nv, (uint32_t)(2 * g_short_row), mass);
      unsigned long long hm[2] = {0, 0};
      if ((rc = read_back(hm, mass.p, s, 2))) return rc;
      no_skew = hm[0] > 0 && hm[1] * 10ull <= hm[0];
    }
    int want_slices = g_sweep_slices >= 8 ? g_sweep_slices : (int)(mib_live / (no_skew ? 4.0 : 1.3) + 0.5);
    // (a shard of G holds 1 / G of the edges but walks the WHOLE message vector: what a slice costs a workgroup whatever it holds --
    // two barriers, the hot-set load, the staging round -- weighs G times more against the gathers it makes cheaper, so a shard wants
    // fewer, larger slices.  Shard 0 of RMAT-26, compute only, ms per iteration by slice count -- of 8: 16 / 20 / 24 / 28 / 32 / 48 / 64 / 96:
    // 1.15 / 1.05 / 1.07 / 1.12 / 1.14 / 1.33 / 1.44 / 1.81; of 4: 16 / 24 / 32 / 96: 1.78 / 1.58 / 1.60 / 2.07; of 2: 24 / 32 / 48 / 96: 2.65 /
    // 2.23 / 2.18 / 2.37 -- about G^-0.75 of the single shard's count; profiles/r06_shard_slice_counts.txt)
    if (shard_slices && g_sweep_slices < 8) want_slices = (int)((double)want_slices / pow((double)G, 0.75) + 0.5);
    want_slices = std::max(16, std::min(GM_MAX_SLICES, want_slices));
    // (an adjacency the sweep cannot take -- edge values that are not 4 bytes wide -- is only ever walked tile by tile: its order stays
    // degree-ranked inside a whole TILE, so that the tile kernels' LDS hot sets hold the tile's busiest vertices, not one slice's)
    const bool sweepable = !keeps_values || D.val_bytes == 4;
    const int sub = (g_sweep_slices != 0 && sweepable) ? std::max(1, std::min(GM_MAX_SLICES / T, (want_slices + T / 2) / T)) : 1;
    const int TS = T * sub;
    GM_LAUNCH_1D(k_tile_of_ranked, nv, s, order, nv, deg, wpre, total, TS, tk_in);
    if ((rc = radix_sort_pairs(tk_in.p, tk_out.p, order.p, order2.p, (size_t)nv, 8, s))) return rc;
    GM_TRY_HIP(hipMemcpyAsync(order, order2, (size_t)nv * 4, hipMemcpyDeviceToDevice, s));
    // where every tile starts in the new order (vertices without edges carry key 255 and sort to the end)
    hipLaunchKernelGGL(k_key_bounds<int64_t>, dim3(1), dim3(256), 0, s, tk_out, (int64_t)nv, TS, bnd);
    int64_t hb[GM_MAX_SLICES + 2];
    if ((rc = read_back(hb, bnd.p, s, (size_t)TS + 1))) return rc;
    if (!shard_slices) {
      for (int t = 0; t <= T; t++) g->tile_base[t] = (int32_t)hb[t * sub];
      g->nslices = sub > 1 ? TS : 0;
      for (int t = 0; t <= TS; t++) g->slice_base[t] = (int32_t)hb[t];
    } else {
      // positions inside an owner's range: slice t takes ceil(n_t / G) of them in every owner
      shard_TS = TS;
      long long pos = 0;
      for (int t = 0; t < TS; t++) { sd.hb[t] = (int32_t)hb[t]; sd.sb[t] = (int32_t)pos; pos += (hb[t + 1] - hb[t] + G - 1) / G; }
      sd.hb[TS] = (int32_t)hb[TS];  // (= vertices with edges; the rest of the list has none)
      sd.sb[TS] = (int32_t)pos;
      const long long ndead = (long long)nv - hb[TS];
      const long long need = pos + (ndead + G - 1) / G;
      S = (int)((need + 63) / 64 * 64);
      vd = G * S;
      g->tile_base[0] = 0; g->tile_base[1] = (int32_t)pos;
      g->nslices = TS;
      for (int t = 0; t <= TS; t++) g->slice_base[t] = sd.sb[t];
      slice_keys = std::move(tk_out);
    }
  }
  g->ntiles = T;
  D.col_tiles = T;
  if ((rc = nod.alloc((size_t)vd))) return rc;
  GM_TRY_HIP(nod.fill(0xff, (size_t)vd, s));  // -1 = unused slot
  if (shard_TS > 0) GM_LAUNCH_1D(k_deal_sliced, nv, s, order, slice_keys, nv, G, S, shard_TS, sd, don, nod);
  else GM_LAUNCH_1D(k_deal, nv, s, order, nv, G, S, don, nod);
  GM_TRY_HIP(hipGetLastError());
  GM_TRY_HIP(hipStreamSynchronize(s));
  {
    long long per = shard_TS > 0 ? (long long)sd.sb[shard_TS] : ((long long)nz + G - 1) / G;
    per = (per + 63) / 64 * 64;
    const long long slice = (G > 1) ? S : nv;
    D.xchg_rows = (int32_t)(per < slice ? per : slice);
    if (D.xchg_rows < 64 && slice >= 64) D.xchg_rows = 64;
  }
  g->dev_of_native = don.release();
  g->native_of_dev = nod.release();
  D.ndevice = vd;
  D.row_lo = (G > 1) ? D.shard * S : 0;
  D.row_hi = (G > 1) ? D.row_lo + S : nv;
  return GM_OK;
}

// does any endpoint (0-based native ids) of these edges have a device id >= limit?
__global__ void __launch_bounds__(kT)
k_any_dev_beyond(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, int64_t nnz, const int32_t* __restrict__ dev_of_native,
                 int limit, unsigned int* __restrict__ flag) {
  const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (k >= nnz) return;
  if (dev_of_native[src[k]] >= limit || dev_of_native[dst[k]] >= limit) *flag = 1u;
}

// edges of a CSR direction back as native (src, dst) pairs, in CSR order
__global__ void __launch_bounds__(kT)
k_csr_to_coo(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, int nrows, int row_base,
             const int32_t* __restrict__ native_of_dev, int rows_are_dst, int32_t* __restrict__ src,
             int32_t* __restrict__ dst) {
  const int row = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const int lane = threadIdx.x & 63;
  const int rn = native_of_dev ? native_of_dev[row_base + row] : row_base + row;
  for (int64_t e = rowptr[row] + lane; e < rowptr[row + 1]; e += 64) {
    int c = colidx[e];
    int cn = native_of_dev ? native_of_dev[c] : c;
    src[e] = rows_are_dst ? cn : rn;
    dst[e] = rows_are_dst ? rn : cn;
  }
}

// tile copies of the edge values from the whole-graph CSR: a row's edges there are the concatenation of its pieces in
// tile order, so `done[r]` (edges of row r already handed to earlier tiles) locates a piece.  One wave per row.
__global__ void __launch_bounds__(kT)
k_tile_vals(const int64_t* __restrict__ rowptr_whole, const unsigned char* __restrict__ vals_whole, const int64_t* __restrict__ rowptr_tile,
            unsigned char* __restrict__ vals_tile, int nrows, int val_bytes, int64_t* __restrict__ done) {
  const int row = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const int64_t a = rowptr_tile[row], len = rowptr_tile[row + 1] - a;
  if (len == 0) return;
  const int64_t from = rowptr_whole[row] + done[row];
  const int64_t bytes = len * val_bytes;
  const unsigned char* src = vals_whole + from * val_bytes;
  unsigned char* dst = vals_tile + a * val_bytes;
  for (int64_t b = threadIdx.x & 63; b < bytes; b += 64) dst[b] = src[b];
  if ((threadIdx.x & 63) == 0) done[row] += len;
}

void free_csr(CsrOwned* c) {
  void* owned[] = {c->rowptr, c->colidx, c->vals, c->rowbits, c->seg_row, c->blk_seg, c->mid_row, c->giant_row, c->gchunk_row, c->gchunk_edge, c->gterm_off, c->umid_row, c->gchunk_state};
  for (void* q : owned)
    if (q) (void)hipFree(q);
  *c = CsrOwned();
}

}  // namespace gm

extern "C" {

int gm_graph_tiles(const gm_graph_t* g, int direction, int* ntiles) {
  if (!g || !ntiles) { gm::set_error("gm_graph_tiles: null argument"); return GM_ERR_INVALID; }
  *ntiles = (direction == GM_DIR_OUT && g->out_tiles && g->ntiles > 1) ? g->ntiles : 1;
  return GM_OK;
}

int gm_graph_sweep(const gm_graph_t* g, gm_sweep_t* out) {
  if (!g || !out) { gm::set_error("gm_graph_sweep: null argument"); return GM_ERR_INVALID; }
  *out = g->sweep;
  return GM_OK;
}

int gm_graph_blocked(const gm_graph_t* g, gm_blocked_t* out) {
  if (!g || !out) { gm::set_error("gm_graph_blocked: null argument"); return GM_ERR_INVALID; }
  *out = g->blocked;
  return GM_OK;
}
int gm_graph_tile(const gm_graph_t* g, int direction, int tile, gm_csr_t* out, const uint32_t** d_prev_bits) {
  if (!g || !out) { gm::set_error("gm_graph_tile: null argument"); return GM_ERR_INVALID; }
  if (direction != GM_DIR_OUT || !g->out_tiles || tile < 0 || tile >= g->ntiles) {
    gm::set_error("gm_graph_tile: no tile %d in direction %d", tile, direction);
    return GM_ERR_INVALID;
  }
  *out = g->out_tiles[tile].view;
  if (d_prev_bits) *d_prev_bits = g->out_tile_prev[tile];
  return GM_OK;
}

// Collective builds (edges_local): a failure on one rank must fail every rank, or the others wait for ever in the next
// collective.  Returns GM_OK only when every rank arrived with rc == GM_OK (one all-reduce of a failure count).
static int agree_on_status(int rc, hipStream_t s) {
  gm::DevArray<uint32_t> w;
  if (w.alloc(16) != GM_OK) return rc != GM_OK ? rc : GM_ERR_NOMEM;  // (cannot even ask: report locally)
  const uint32_t mine = rc != GM_OK ? 1u : 0u;
  uint32_t total = 0;
  if (hipMemcpyAsync(w.p, &mine, 4, hipMemcpyHostToDevice, s) != hipSuccess) return rc != GM_OK ? rc : GM_ERR_HIP;
  int rc2 = gm::dist_all_reduce_sum_u32(w, 1, s);
  if (rc2 != GM_OK) return rc != GM_OK ? rc : rc2;
  if (hipMemcpyAsync(&total, w.p, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return rc != GM_OK ? rc : GM_ERR_HIP;
  if (rc != GM_OK) return rc;
  if (total != 0) { gm::set_error("gm_graph_create: the distributed build failed on %u other rank(s)", total); return GM_ERR_INVALID; }
  return GM_OK;
}

int gm_graph_create(gm_graph_t** gout, const gm_graph_desc_t* desc, int64_t nnz, const int32_t* src,
                    const int32_t* dst, const void* val, gm_stream_t stream) {
  if (!gout || !desc) { gm::set_error("gm_graph_create: null argument"); return GM_ERR_INVALID; }
  *gout = nullptr;
  if (desc->nvertices <= 0 || nnz < 0 || desc->nparts <= 0 || desc->row_lo < 0 || desc->row_hi > desc->nvertices ||
      desc->row_lo > desc->row_hi || (desc->directions & (GM_DIR_OUT | GM_DIR_IN)) == 0 || desc->val_bytes < 0 ||
      (nnz > 0 && (!src || !dst))) {
    gm::set_error("gm_graph_create: invalid descriptor (nv=%d nnz=%lld nparts=%d rows=[%d,%d) dirs=%d)", desc->nvertices,
                  (long long)nnz, desc->nparts, desc->row_lo, desc->row_hi, desc->directions);
    return GM_ERR_INVALID;
  }
  if (desc->layout == GM_LAYOUT_NATIVE &&
      ((desc->row_lo & 63) != 0 || ((desc->row_hi & 63) != 0 && desc->row_hi != desc->nvertices))) {
    gm::set_error("gm_graph_create: shard boundaries must be multiples of 64 (got [%d,%d))", desc->row_lo, desc->row_hi);
    return GM_ERR_INVALID;
  }
  if (desc->layout != GM_LAYOUT_NATIVE && desc->layout != GM_LAYOUT_DEGREE) {
    gm::set_error("gm_graph_create: unknown layout %d", desc->layout);
    return GM_ERR_INVALID;
  }
  if (desc->layout == GM_LAYOUT_DEGREE && (desc->nshards < 1 || desc->shard < 0 || desc->shard >= desc->nshards)) {
    gm::set_error("gm_graph_create: invalid shard %d of %d", desc->shard, desc->nshards);
    return GM_ERR_INVALID;
  }
  if (nnz >= (1ll << 32)) { gm::set_error("gm_graph_create: more than 2^32-1 edges per call is unsupported"); return GM_ERR_UNSUPPORTED; }
  if (desc->edges_local) {
    int wr = 0, wn = 0;
    if (desc->layout != GM_LAYOUT_DEGREE) { gm::set_error("gm_graph_create: edges_local needs GM_LAYOUT_DEGREE"); return GM_ERR_INVALID; }
    if (desc->nshards > 65535) { gm::set_error("gm_graph_create: edges_local supports at most 65535 shards"); return GM_ERR_UNSUPPORTED; }
    if (!gm::dist_world(&wr, &wn) || wn != desc->nshards || wr != desc->shard) {
      gm::set_error("gm_graph_create: edges_local is a collective over the gm_dist communicator (have rank %d of %d, graph is shard %d of %d)",
                    wr, wn, desc->shard, desc->nshards);
      return GM_ERR_INVALID;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  gm_graph* g = new gm_graph();
  memset((void*)g, 0, sizeof(*g));
  g->desc = *desc;
  g->out = gm::CsrOwned();
  g->in = gm::CsrOwned();

  gm::DevArray<int32_t> usrc, udst;
  gm::DevBuf uval;
  const int32_t* d_src = src;
  const int32_t* d_dst = dst;
  const void* d_val = val;
  int rc = GM_OK;
  if (!desc->ids_on_device && nnz > 0) {
    if ((rc = usrc.alloc((size_t)nnz)) || (rc = udst.alloc((size_t)nnz))) { if (desc->edges_local) (void)agree_on_status(rc, s); delete g; return rc; }
    hipError_t e1 = hipMemcpyAsync(usrc.p, src, (size_t)nnz * 4, hipMemcpyHostToDevice, s);
    hipError_t e2 = hipMemcpyAsync(udst.p, dst, (size_t)nnz * 4, hipMemcpyHostToDevice, s);
    if (e1 != hipSuccess || e2 != hipSuccess) { gm::set_error("edge upload failed"); if (desc->edges_local) (void)agree_on_status(GM_ERR_HIP, s); delete g; return GM_ERR_HIP; }
    d_src = usrc;
    d_dst = udst;
    if (val && desc->val_bytes > 0) {
      if ((rc = uval.alloc((size_t)nnz * desc->val_bytes))) { if (desc->edges_local) (void)agree_on_status(rc, s); delete g; return rc; }
      if (hipMemcpyAsync(uval.p, val, (size_t)nnz * desc->val_bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
        gm::set_error("edge value upload failed"); if (desc->edges_local) (void)agree_on_status(GM_ERR_HIP, s); delete g; return GM_ERR_HIP;
      }
      d_val = uval.p;
    }
  }
  if (nnz > 0) {  // every id must name a vertex: 1..nvertices (0..nvertices-1 when ids_are_native)
    gm::DevArray<unsigned long long> badc;
    if ((rc = badc.alloc(2))) { if (desc->edges_local) (void)agree_on_status(rc, s); delete g; return rc; }
    const unsigned long long init[2] = {0ull, ~0ull};
    const int lo = desc->ids_are_native ? 0 : 1, hi = desc->ids_are_native ? desc->nvertices - 1 : desc->nvertices;
    unsigned long long bad[2] = {0ull, 0ull};
    if (hipMemcpyAsync(badc.p, init, 16, hipMemcpyHostToDevice, s) != hipSuccess) { gm::set_error("edge id check: upload failed"); if (desc->edges_local) (void)agree_on_status(GM_ERR_HIP, s); delete g; return GM_ERR_HIP; }
    hipLaunchKernelGGL(gm::k_validate_ids, dim3(gm::grid_for(nnz)), dim3(gm::kT), 0, s, d_src, d_dst, nnz, lo, hi, badc);
    if (hipMemcpyAsync(bad, badc.p, 16, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
      gm::set_error("edge id check failed: %s", hipGetErrorString(hipGetLastError()));
      if (desc->edges_local) (void)agree_on_status(GM_ERR_HIP, s);
      delete g;
      return GM_ERR_HIP;
    }
    if (bad[0] != 0) {
      gm::set_error("gm_graph_create: %llu edge(s) name a vertex outside [%d, %d] (first: edge %llu); ids are %s", bad[0], lo, hi,
                    bad[1] - 1ull, desc->ids_are_native ? "0-based native ids" : "1-based vertex ids as in the .mtx file");
      rc = GM_ERR_INVALID;
    }
  }
  if (desc->edges_local) rc = agree_on_status(rc, s);  // (bad ids / failed uploads on ANY rank stop all of them here)
  if (rc != GM_OK) { delete g; return rc; }
  g->desc.ndevice = desc->nvertices;
  g->desc.xchg_rows = desc->row_hi - desc->row_lo;
  g->ntiles = 1;
  if (desc->layout == GM_LAYOUT_DEGREE) rc = gm::build_degree_layout(g, nnz, d_src, d_dst, s, desc->val_bytes > 0 && d_val != nullptr);
  else g->desc.col_tiles = 1;
  if (rc != GM_OK) { gm_graph_destroy(g); return rc; }
  if (desc->edges_local) {
    if (desc->directions & GM_DIR_OUT) rc = gm::build_direction_local(g, 1, nnz, d_src, d_dst, d_val, s, &g->out);
    if (rc == GM_OK && (desc->directions & GM_DIR_IN)) rc = gm::build_direction_local(g, 0, nnz, d_src, d_dst, d_val, s, &g->in);
  } else {
    if (desc->directions & GM_DIR_OUT) rc = gm::build_direction(g, 1, nnz, d_src, d_dst, d_val, s, &g->out);
    if (rc == GM_OK && (desc->directions & GM_DIR_IN)) rc = gm::build_direction(g, 0, nnz, d_src, d_dst, d_val, s, &g->in);
  }
  if (rc != GM_OK) { gm_graph_destroy(g); return rc; }
  if (g->out.present && g->in.present) {
    const int nw = (g->desc.row_hi - g->desc.row_lo + 31) / 32 + 2;
    if (hipMalloc((void**)&g->rowbits_all, (size_t)nw * 4) != hipSuccess) { gm::set_error("rowbits alloc failed"); gm_graph_destroy(g); return GM_ERR_NOMEM; }
    hipLaunchKernelGGL(gm::k_or_words<uint32_t>, dim3(gm::grid_for(nw)), dim3(gm::kT), 0, s, g->out.rowbits,
                       g->in.rowbits, g->rowbits_all, nw);
  }
  if (hipStreamSynchronize(s) != hipSuccess) { gm::set_error("graph build: stream sync failed"); gm_graph_destroy(g); return GM_ERR_HIP; }
  void* unused[4];
  if ((rc = gm_graph_run_resources(g, &unused[0], &unused[1], &unused[2], &unused[3])) != GM_OK) { gm_graph_destroy(g); return rc; }
  void* flag = nullptr;
  if (gm_graph_workspace(g, GM_WS_FLAGS, 4096, &flag) == GM_OK) gm::warm_program_kernels(flag);
  *gout = g;
  return GM_OK;
}

int gm_graph_run_resources(gm_graph_t* g, void** aux_stream, void** fork_event, void** join_event, void** pinned) {
  if (!g || !aux_stream || !fork_event || !join_event || !pinned) { gm::set_error("gm_graph_run_resources: null argument"); return GM_ERR_INVALID; }
  if (!g->aux_stream) {
    GM_TRY_HIP(hipStreamCreateWithFlags(&g->aux_stream, hipStreamNonBlocking));
    GM_TRY_HIP(hipEventCreateWithFlags(&g->aux_fork, hipEventDisableTiming));
    GM_TRY_HIP(hipEventCreateWithFlags(&g->aux_join, hipEventDisableTiming));
    GM_TRY_HIP(hipHostMalloc(&g->pinned_flag, 4096, hipHostMallocDefault));
    memset(g->pinned_flag, 0, 4096);
    // first device-to-pinned-host copy of a process sets up the copy path (milliseconds): do it now
    void* d = nullptr;
    GM_TRY_HIP(hipMalloc(&d, 64));
    GM_TRY_HIP(hipMemsetAsync(d, 0, 64, 0));
    GM_TRY_HIP(hipMemcpyAsync(g->pinned_flag, d, 64, hipMemcpyDeviceToHost, 0));
    GM_TRY_HIP(hipStreamSynchronize(0));
    (void)hipFree(d);
  }
  *aux_stream = (void*)g->aux_stream;
  *fork_event = (void*)g->aux_fork;
  *join_event = (void*)g->aux_join;
  *pinned = g->pinned_flag;
  return GM_OK;
}

int gm_graph_destroy(gm_graph_t* g) {
  if (!g) return GM_OK;
  gm::free_csr(&g->out);
  gm::free_csr(&g->in);
  if (g->dev_of_native) (void)hipFree(g->dev_of_native);
  if (g->native_of_dev) (void)hipFree(g->native_of_dev);
  if (g->rowbits_all) (void)hipFree(g->rowbits_all);
  gm::free_tiles(g);
  gm::free_native_exchange(g);
  for (int i = 0; i < GM_WS_SLOTS; i++)
    if (g->ws[i] && !g->ws_external[i]) (void)hipFree(g->ws[i]);
  if (g->aux_stream) {
    (void)hipStreamSynchronize(g->aux_stream);
    (void)hipStreamDestroy(g->aux_stream);
    (void)hipEventDestroy(g->aux_fork);
    (void)hipEventDestroy(g->aux_join);
    (void)hipHostFree(g->pinned_flag);
  }
  delete g;
  return GM_OK;
}

int gm_graph_desc(const gm_graph_t* g, gm_graph_desc_t* out) {
  if (!g || !out) { gm::set_error("gm_graph_desc: null argument"); return GM_ERR_INVALID; }
  *out = g->desc;
  return GM_OK;
}

int gm_graph_csr(const gm_graph_t* g, int direction, gm_csr_t* out) {
  if (!g || !out) { gm::set_error("gm_graph_csr: null argument"); return GM_ERR_INVALID; }
  const gm::CsrOwned* c = direction == GM_DIR_OUT ? &g->out : direction == GM_DIR_IN ? &g->in : nullptr;
  if (!c || !c->present) { gm::set_error("gm_graph_csr: direction %d not built", direction); return GM_ERR_INVALID; }
  *out = c->view;
  return GM_OK;
}

int gm_graph_relayout_like(gm_graph_t* g, const gm_graph_t* like, gm_stream_t stream) {
  if (!g || !like) { gm::set_error("gm_graph_relayout_like: null graph"); return GM_ERR_INVALID; }
  if (g == like) return GM_OK;
  const gm_graph_desc_t &a = g->desc, &b = like->desc;
  // Sharded graphs (one process per shard, both graphs cut the same way): a COLLECTIVE over the gm_dist communicator.
  // In the other graph's order a row may belong to another shard, so every rank hands the edges it holds back to the
  // distributed build (build_direction_local: the owner of each edge's row under the adopted order receives it).
  const bool sharded = a.nshards > 1 || b.nshards > 1;
  if (sharded) {
    int wr = 0, wn = 0;
    if (a.nvertices != b.nvertices || a.nparts != b.nparts || a.nshards != b.nshards || a.shard != b.shard || a.ndevice != b.ndevice ||
        a.row_lo != b.row_lo || a.row_hi != b.row_hi || a.layout != GM_LAYOUT_DEGREE || b.layout != GM_LAYOUT_DEGREE ||
        !gm::dist_world(&wr, &wn) || wn != a.nshards || wr != a.shard) {
      gm::set_error("gm_graph_relayout_like: sharded graphs must be the same shard of the same cut, with the gm_dist communicator up");
      return GM_ERR_INVALID;
    }
  } else if (a.nvertices != b.nvertices || a.nparts != b.nparts || a.row_lo != 0 || a.row_hi != a.ndevice || b.row_lo != 0 ||
             b.row_hi != b.ndevice || a.ndevice != b.ndevice) {
    gm::set_error("gm_graph_relayout_like: graphs must have the same vertices and the same cut");
    return GM_ERR_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  gm::CsrOwned* from = g->in.present ? &g->in : &g->out;
  const int64_t nnz = from->view.nnz;
  gm::DevArray<int32_t> src, dst;
  int rc;
  if ((rc = src.alloc((size_t)nnz)) || (rc = dst.alloc((size_t)nnz))) return rc;
  if (from->view.nrows > 0)
    hipLaunchKernelGGL(gm::k_csr_to_coo, dim3((from->view.nrows + 3) / 4), dim3(gm::kT), 0, s, from->view.rowptr,
                       from->view.colidx, from->view.nrows, from->view.row_base, g->native_of_dev,
                       from == &g->out ? 1 : 0, src, dst);
  GM_TRY_HIP(hipGetLastError());
  // the edge values travel in the same (CSR) order; keep them alive while rebuilding
  void* vals = from->vals;
  from->vals = nullptr;
  const int val_bytes = from->view.val_bytes;
  gm::CsrOwned old_out = g->out, old_in = g->in;
  g->out = gm::CsrOwned();
  g->in = gm::CsrOwned();
  // adopt the other graph's device order
  if (g->dev_of_native) (void)hipFree(g->dev_of_native);
  if (g->native_of_dev) (void)hipFree(g->native_of_dev);
  g->dev_of_native = nullptr;
  g->native_of_dev = nullptr;
  if (like->dev_of_native) {
    GM_TRY_HIP(hipMalloc((void**)&g->dev_of_native, (size_t)b.nvertices * 4));
    GM_TRY_HIP(hipMalloc((void**)&g->native_of_dev, (size_t)b.ndevice * 4));
    GM_TRY_HIP(hipMemcpyAsync(g->dev_of_native, like->dev_of_native, (size_t)b.nvertices * 4, hipMemcpyDeviceToDevice, s));
    GM_TRY_HIP(hipMemcpyAsync(g->native_of_dev, like->native_of_dev, (size_t)b.ndevice * 4, hipMemcpyDeviceToDevice, s));
  }
  g->desc.layout = b.layout;
  // ... and its column tiles (the tile of a column is a function of its device id) -- but only if every vertex that has
  // an edge in g lies inside like's tiles: a vertex without edges in `like` sits behind the last tile in like's order
  // (device id >= tile_base[T]) whatever its native id, so with such columns the tiles would no longer be contiguous
  // native ranges -- the tile-after-tile fold would leave the ascending-native-column order and the tile copies of the
  // edge values would not line up with the whole CSR.  Such a graph simply keeps the untiled multiply.
  gm::free_tiles(g);
  int like_tiles = like->ntiles > 1 ? like->ntiles : 1;
  if (sharded) like_tiles = 1;
  if (like_tiles > 1 && nnz > 0) {
    gm::DevArray<unsigned int> flag;
    if ((rc = flag.alloc(1))) return rc;
    GM_TRY_HIP(flag.fill(0, 1, s));
    hipLaunchKernelGGL(gm::k_any_dev_beyond, dim3(gm::grid_for(nnz)), dim3(gm::kT), 0, s, src, dst, nnz,
                       like->dev_of_native, like->tile_base[like_tiles], flag);
    unsigned int outside = 0;
    if ((rc = gm::read_back(&outside, flag.p, s))) return rc;
    if (outside) like_tiles = 1;
  }
  g->ntiles = like_tiles;
  memcpy(g->tile_base, like->tile_base, sizeof(g->tile_base));
  // (... and the finer cut of the adopted order: the slices are native ranges of LIKE's order -- this graph's own cuts, made for the order it
  // had, are not: a row folded slice by slice through them would leave the ascending-native-column order, and the column-blocked stream,
  // whose "first edge of the row" is the CSR's first, would assign it in the middle of a row)
  g->nslices = like_tiles > 1 ? like->nslices : 0;
  memcpy(g->slice_base, like->slice_base, sizeof(g->slice_base));
  g->nlive = like->nlive;
  g->desc.col_tiles = g->ntiles;
  // the other graph's order ranks ITS edges: this graph's vertices with edges may sit anywhere in it
  g->desc.xchg_rows = b.row_hi - b.row_lo;
  const int saved_native = g->desc.ids_are_native, saved_vb = g->desc.val_bytes;
  g->desc.ids_are_native = 1;
  g->desc.val_bytes = val_bytes;
  rc = GM_OK;
  if (sharded) {  // this rank's edges (the rows it owned under the old order) go to their new owners
    if (g->desc.directions & GM_DIR_OUT) rc = gm::build_direction_local(g, 1, nnz, src, dst, vals, s, &g->out);
    if (rc == GM_OK && (g->desc.directions & GM_DIR_IN)) rc = gm::build_direction_local(g, 0, nnz, src, dst, vals, s, &g->in);
  } else {
    if (g->desc.directions & GM_DIR_OUT) rc = gm::build_direction(g, 1, nnz, src, dst, vals, s, &g->out);
    if (rc == GM_OK && (g->desc.directions & GM_DIR_IN)) rc = gm::build_direction(g, 0, nnz, src, dst, vals, s, &g->in);
  }
  g->desc.ids_are_native = saved_native;
  g->desc.val_bytes = saved_vb;
  if (vals) (void)hipFree(vals);
  gm::free_csr(&old_out);
  gm::free_csr(&old_in);
  memset(g->split_memo, 0, sizeof(g->split_memo));  // answers about the old adjacency
  memset(g->note_set, 0, sizeof(g->note_set));
  if (rc != GM_OK) return rc;
  if (g->rowbits_all && g->out.present && g->in.present) {
    const int nw = (g->desc.row_hi - g->desc.row_lo + 31) / 32 + 2;
    hipLaunchKernelGGL(gm::k_or_words<uint32_t>, dim3(gm::grid_for(nw)), dim3(gm::kT), 0, s, g->out.rowbits,
                       g->in.rowbits, g->rowbits_all, nw);
  }
  GM_TRY_HIP(hipStreamSynchronize(s));
  return GM_OK;
}

int gm_graph_rowbits_all(const gm_graph_t* g, const uint32_t** d_bits) {
  if (!g || !d_bits) { gm::set_error("gm_graph_rowbits_all: null argument"); return GM_ERR_INVALID; }
  if (!g->rowbits_all) { gm::set_error("gm_graph_rowbits_all: graph was not built with both directions"); return GM_ERR_INVALID; }
  *d_bits = g->rowbits_all;
  return GM_OK;
}

int gm_graph_maps(const gm_graph_t* g, const int32_t** d_dev_of_native, const int32_t** d_native_of_dev) {
  if (!g) { gm::set_error("gm_graph_maps: null graph"); return GM_ERR_INVALID; }
  if (d_dev_of_native) *d_dev_of_native = g->dev_of_native;
  if (d_native_of_dev) *d_native_of_dev = g->native_of_dev;
  return GM_OK;
}

int gm_graph_maps_to_host(const gm_graph_t* g, int32_t* h_dev_of_native, int32_t* h_native_of_dev) {
  if (!g) { gm::set_error("gm_graph_maps_to_host: null graph"); return GM_ERR_INVALID; }
  const int nv = g->desc.nvertices, vd = g->desc.ndevice;
  if (h_dev_of_native) {
    if (g->dev_of_native) GM_TRY_HIP(hipMemcpy(h_dev_of_native, g->dev_of_native, (size_t)nv * 4, hipMemcpyDeviceToHost));
    else for (int i = 0; i < nv; i++) h_dev_of_native[i] = i;
  }
  if (h_native_of_dev) {
    if (g->native_of_dev) GM_TRY_HIP(hipMemcpy(h_native_of_dev, g->native_of_dev, (size_t)vd * 4, hipMemcpyDeviceToHost));
    else for (int i = 0; i < vd; i++) h_native_of_dev[i] = i;
  }
  return GM_OK;
}

int gm_graph_csr_to_host(const gm_graph_t* g, int direction, int64_t* h_rowptr, int32_t* h_colidx, void* h_vals) {
  gm_csr_t v;
  int rc = gm_graph_csr(g, direction, &v);
  if (rc) return rc;
  if (h_rowptr) GM_TRY_HIP(hipMemcpy(h_rowptr, v.rowptr, (size_t)(v.nrows + 1) * 8, hipMemcpyDeviceToHost));
  if (h_colidx && v.nnz) GM_TRY_HIP(hipMemcpy(h_colidx, v.colidx, (size_t)v.nnz * 4, hipMemcpyDeviceToHost));
  if (h_vals && v.vals && v.nnz) GM_TRY_HIP(hipMemcpy(h_vals, v.vals, (size_t)v.nnz * v.val_bytes, hipMemcpyDeviceToHost));
  return GM_OK;
}

int gm_graph_set_vals(gm_graph_t* g, int direction, const void* h_vals) {
  if (!g || !h_vals) { gm::set_error("gm_graph_set_vals: null argument"); return GM_ERR_INVALID; }
  gm::CsrOwned* c = direction == GM_DIR_OUT ? &g->out : direction == GM_DIR_IN ? &g->in : nullptr;
  if (!c || !c->present || !c->vals) { gm::set_error("gm_graph_set_vals: direction %d has no edge values", direction); return GM_ERR_INVALID; }
  if (c->view.nnz) GM_TRY_HIP(hipMemcpy(c->vals, h_vals, (size_t)c->view.nnz * c->view.val_bytes, hipMemcpyHostToDevice));
  return direction == GM_DIR_OUT ? gm_graph_sync_tile_vals(g, nullptr) : GM_OK;
}

int gm_graph_sync_tile_vals(gm_graph_t* g, gm_stream_t stream) {
  if (!g) { gm::set_error("gm_graph_sync_tile_vals: null graph"); return GM_ERR_INVALID; }
  if (!g->out.present || !g->out.vals) return GM_OK;
  hipStream_t s = (hipStream_t)stream;
  {  // the sweep's copies of the values (gm_sweep_t.sval / lval), through the CSR positions its entries came from
    const gm_sweep_t& S = g->sweep;
    if (S.nrows > 0 && S.val_bytes == 4 && S.sval && S.src_pos && S.nentries > 0)
      hipLaunchKernelGGL(gm::k_sweep_sync_vals, dim3(gm::grid_for(S.nentries)), dim3(gm::kT), 0, s, S.src_pos, (size_t)S.nentries, (const uint32_t*)g->out.vals,
                         const_cast<uint32_t*>(S.sval));
    if (S.nrows > 0 && S.val_bytes == 4 && S.gval && S.gsrc_pos && S.ngiant_edges > 0)
      hipLaunchKernelGGL(gm::k_sweep_sync_vals, dim3(gm::grid_for(S.ngiant_edges)), dim3(gm::kT), 0, s, S.gsrc_pos, (size_t)S.ngiant_edges, (const uint32_t*)g->out.vals,
                         const_cast<uint32_t*>(S.gval));
    if (S.nrows > 0 && S.val_bytes == 4 && S.lval && S.lsrc_pos && S.nedges_long > 0)
      hipLaunchKernelGGL(gm::k_sweep_sync_vals, dim3(gm::grid_for(S.nedges_long)), dim3(gm::kT), 0, s, S.lsrc_pos, (size_t)S.nedges_long, (const uint32_t*)g->out.vals,
                         const_cast<uint32_t*>(S.lval));
  }
  {  // ... and the column-blocked stream's (gm_blocked_t.eval)
    const gm_blocked_t& B = g->blocked;
    if (B.nrows > 0 && B.val_bytes == 4 && B.eval && B.epos && B.nentries > 0)
      hipLaunchKernelGGL(gm::k_sweep_sync_vals, dim3(gm::grid_for(B.nentries)), dim3(gm::kT), 0, s, B.epos, (size_t)B.nentries, (const uint32_t*)g->out.vals,
                         const_cast<uint32_t*>(B.eval));
  }
  if (g->ntiles <= 1 || !g->out_tiles) { GM_TRY_HIP(hipGetLastError()); GM_TRY_HIP(hipStreamSynchronize(s)); return GM_OK; }
  const int nrows = g->out.view.nrows, vb = g->out.view.val_bytes;
  gm::DevArray<int64_t> done;
  int rc;
  if ((rc = done.alloc((size_t)nrows + 1))) return rc;
  GM_TRY_HIP(done.fill(0, (size_t)nrows + 1, s));
  // (rows of at most tile_min_row edges have no tile pieces; the tiled rows' pieces cover them completely)
  for (int t = 0; t < g->ntiles; t++) {
    gm::CsrOwned& T = g->out_tiles[t];
    if (!T.vals || T.view.nnz == 0) continue;
    hipLaunchKernelGGL(gm::k_tile_vals, dim3((nrows + gm::kT / 64 - 1) / (gm::kT / 64)), dim3(gm::kT), 0, s, g->out.rowptr,
                       (const unsigned char*)g->out.vals, (const int64_t*)T.rowptr, (unsigned char*)T.vals, nrows, vb, done);
  }
  GM_TRY_HIP(hipGetLastError());
  GM_TRY_HIP(hipStreamSynchronize(s));
  return GM_OK;
}

int gm_graph_workspace(gm_graph_t* g, int slot, size_t bytes, void** d_ptr) {
  if (!g || slot < 0 || slot >= GM_WS_SLOTS || !d_ptr) { gm::set_error("gm_graph_workspace: invalid argument"); return GM_ERR_INVALID; }
  if (g->ws_bytes[slot] < bytes) {
    if (g->ws_external[slot]) {
      gm::set_error("adopted workspace slot %d is too small (%zu < %zu bytes)", slot, g->ws_bytes[slot], bytes);
      return GM_ERR_INVALID;
    }
    if (g->ws[slot]) (void)hipFree(g->ws[slot]);
    g->ws[slot] = nullptr;
    g->ws_bytes[slot] = 0;
    hipError_t e = hipMalloc(&g->ws[slot], bytes);
    if (e != hipSuccess) { gm::set_error("workspace hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return GM_ERR_NOMEM; }
    g->ws_bytes[slot] = bytes;
  }
  *d_ptr = g->ws[slot];
  return GM_OK;
}

int gm_graph_note_set(gm_graph_t* g, int slot, int64_t value) {
  if (!g || slot < 0 || slot >= GM_NOTE_SLOTS) { gm::set_error("gm_graph_note_set: invalid argument"); return GM_ERR_INVALID; }
  g->note_val[slot] = value;
  g->note_set[slot] = 1;
  return GM_OK;
}
int gm_graph_note_get(const gm_graph_t* g, int slot, int64_t* value) {
  if (!g || slot < 0 || slot >= GM_NOTE_SLOTS || !value || !g->note_set[slot]) return GM_ERR_INVALID;
  *value = g->note_val[slot];
  return GM_OK;
}

int gm_graph_workspace_info(const gm_graph_t* g, int slot, void** d_ptr, size_t* bytes, int* external) {
  if (!g || slot < 0 || slot >= GM_WS_SLOTS || !d_ptr || !bytes || !external) { gm::set_error("gm_graph_workspace_info: invalid argument"); return GM_ERR_INVALID; }
  *d_ptr = g->ws[slot];
  *bytes = g->ws_bytes[slot];
  *external = g->ws_external[slot];
  return GM_OK;
}

int gm_graph_split(const gm_graph_t* g, int direction, int head_permille, int32_t* row_split, int32_t* blk_split,
                   int32_t* mid_split) {
  if (!g || !row_split || !blk_split || !mid_split || head_permille < 1 || head_permille > 999) { gm::set_error("gm_graph_split: invalid argument"); return GM_ERR_INVALID; }
  const gm::CsrOwned* c = direction == GM_DIR_OUT ? &g->out : direction == GM_DIR_IN ? &g->in : nullptr;
  if (!c || !c->present) { gm::set_error("gm_graph_split: direction %d not built", direction); return GM_ERR_INVALID; }
  const gm_csr_t& A = c->view;
  gm_graph::SplitMemo* memo = const_cast<gm_graph::SplitMemo*>(g->split_memo[direction == GM_DIR_OUT ? 0 : 1]);
  for (int k = 0; k < 2; k++)
    if (memo[k].valid && memo[k].permille == head_permille && memo[k].asked == *row_split) {
      *row_split = memo[k].rs; *blk_split = memo[k].bs; *mid_split = memo[k].ms;
      return GM_OK;
    }
  const int32_t asked = *row_split;
  auto rd64 = [&](const int64_t* p, int64_t i, int64_t* out) { return hipMemcpy(out, p + i, 8, hipMemcpyDeviceToHost); };
  auto rd32 = [&](const int32_t* p, int64_t i, int32_t* out) { return hipMemcpy(out, p + i, 4, hipMemcpyDeviceToHost); };
  const int64_t target = (A.nnz * head_permille + 999) / 1000;
  // smallest multiple of 64 (capped at nrows) with rowptr[row] >= target
  int64_t lo = 0, hi = ((int64_t)A.nrows + 63) / 64;
  while (lo < hi) {
    const int64_t mid = (lo + hi) / 2;
    const int64_t r = mid * 64 < A.nrows ? mid * 64 : A.nrows;
    int64_t v = 0;
    GM_TRY_HIP(rd64(A.rowptr, r, &v));
    if (v >= target) hi = mid; else lo = mid + 1;
  }
  int64_t rs = lo * 64 < A.nrows ? lo * 64 : A.nrows;
  if (*row_split > 0) rs = (int64_t)(*row_split) < A.nrows ? (int64_t)(*row_split) / 64 * 64 : A.nrows;  // caller's choice
  // first row-block whose rows end beyond rs
  int64_t bl = 0, bh = A.nblk;
  while (bl < bh) {
    const int64_t mid = (bl + bh) / 2;
    int32_t sg = 0, r1 = 0;
    GM_TRY_HIP(rd32(A.blk_seg, mid, &sg));
    GM_TRY_HIP(rd32(A.seg_row, (int64_t)sg + 1, &r1));
    if ((int64_t)r1 > rs) bh = mid; else bl = mid + 1;
  }
  int64_t ml = 0, mh = A.nmid;
  while (ml < mh) {
    const int64_t mid = (ml + mh) / 2;
    int32_t r = 0;
    GM_TRY_HIP(rd32(A.mid_row, mid, &r));
    if ((int64_t)r >= rs) mh = mid; else ml = mid + 1;
  }
  if (A.ngiant > 0) {
    int32_t last = 0;
    GM_TRY_HIP(rd32(A.giant_row, (int64_t)A.ngiant - 1, &last));
    if ((int64_t)last >= rs) { gm::set_error("gm_graph_split: a giant row lies in the tail"); return GM_ERR_INVALID; }
  }
  *row_split = (int32_t)rs;
  *blk_split = (int32_t)bl;
  *mid_split = (int32_t)ml;
  gm_graph::SplitMemo& m = memo[asked == 0 ? 0 : 1];
  m.valid = 1; m.permille = head_permille; m.asked = asked; m.rs = (int32_t)rs; m.bs = (int32_t)bl; m.ms = (int32_t)ml;
  return GM_OK;
}

int gm_graph_adopt_workspace(gm_graph_t* g, int slot, void* d_ptr, size_t bytes) {
  if (!g || slot < 0 || slot >= GM_WS_SLOTS) { gm::set_error("gm_graph_adopt_workspace: invalid argument"); return GM_ERR_INVALID; }
  if (g->ws[slot] && !g->ws_external[slot]) (void)hipFree(g->ws[slot]);
  g->ws[slot] = d_ptr;
  g->ws_bytes[slot] = d_ptr ? bytes : 0;
  g->ws_external[slot] = d_ptr ? 1 : 0;
  return GM_OK;
}

int gm_graph_set_exchange(gm_graph_t* g, gm_exchange_fn fn, void* ctx) {
  if (!g) { gm::set_error("gm_graph_set_exchange: null graph"); return GM_ERR_INVALID; }
  g->xfn = fn;
  g->xctx = ctx;
  g->xcaps = 0;
  return GM_OK;
}
int gm_graph_set_exchange_caps(gm_graph_t* g, int caps) {
  if (!g) { gm::set_error("gm_graph_set_exchange_caps: null graph"); return GM_ERR_INVALID; }
  g->xcaps = caps;
  return GM_OK;
}
int gm_graph_exchange_caps(const gm_graph_t* g) { return (g && g->xfn) ? g->xcaps : 0; }
int gm_graph_has_exchange(const gm_graph_t* g) { return (g && g->xfn) ? 1 : 0; }
int gm_graph_exchange(gm_graph_t* g, int kind, void* d_ptr, int64_t elt_bytes, uint32_t* d_bits, int* h_flag) {
  if (!g || !g->xfn) return GM_OK;
  return g->xfn(g->xctx, kind, d_ptr, elt_bytes, d_bits, h_flag);
}
int gm_graph_enable_timing(gm_graph_t* g, int on) {
  if (!g) return GM_ERR_INVALID;
  g->timing = on ? 1 : 0;
  return GM_OK;
}
int gm_graph_timing_enabled(const gm_graph_t* g) { return g ? g->timing : 0; }
int gm_graph_record_stats(gm_graph_t* g, const gm_run_stats_t* st) {
  if (!g || !st) return GM_ERR_INVALID;
  g->stats = *st;
  return GM_OK;
}
int gm_graph_last_stats(const gm_graph_t* g, gm_run_stats_t* out) {
  if (!g || !out) return GM_ERR_INVALID;
  *out = g->stats;
  return GM_OK;
}

}  // extern "C"
