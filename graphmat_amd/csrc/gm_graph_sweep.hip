// gm_graph_sweep.hip -- builds gm_sweep_t: the rows of more than short_row edges that are not giant laid out for the row-stationary
// sweep (kernels.hpp: k_spmv_sell), the short rows as its stream groups, and the giant rows' edges by slice.
// build_sweep at the end of the file lists the stages; every stage is a function of its own above it.
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "gm_build.hpp"

namespace gm {

using u64 = unsigned long long;

// the sorts that other units use too (gm_build.hpp)
template int radix_sort_pairs_desc<uint32_t, int32_t>(const uint32_t*, uint32_t*, const int32_t*, int32_t*, size_t, unsigned, hipStream_t);
template int radix_sort_pairs<unsigned long long, uint32_t>(const unsigned long long*, unsigned long long*, const uint32_t*, uint32_t*, size_t, unsigned, hipStream_t);
template int radix_sort_pairs<uint8_t, uint32_t>(const uint8_t*, uint8_t*, const uint32_t*, uint32_t*, size_t, unsigned, hipStream_t);

// ---- gm_graph_sweep: the rows of more than short_row edges that are not giant, laid out for kernels.hpp: k_spmv_sell ----------
// (graphmat_hip.h: gm_sweep_t; prototype and measurements: tools/sell_bench.hip, profiles/r05_sell_prototype*.txt)
__global__ void __launch_bounds__(kT)
k_sweep_flag(const int64_t* __restrict__ rowptr, int nrows, int short_row, unsigned char* __restrict__ flag) {
  const int r = blockIdx.x * kT + threadIdx.x;
  if (r < nrows) flag[r] = (rowptr[r + 1] - rowptr[r] > short_row) ? 1 : 0;
}
__global__ void __launch_bounds__(kT) k_sweep_unflag(const int32_t* __restrict__ list, int n, unsigned char* __restrict__ flag) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i < n) flag[list[i]] = 0;
}
__global__ void __launch_bounds__(kT)
k_sweep_lens(const int32_t* __restrict__ rows, int n, const int64_t* __restrict__ rowptr, uint32_t* __restrict__ len) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i < n) len[i] = (uint32_t)(rowptr[rows[i] + 1] - rowptr[rows[i]]);
}
__global__ void __launch_bounds__(kT) k_sweep_widen(const uint32_t* __restrict__ a, int n, unsigned long long* __restrict__ o) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i < n) o[i] = a[i];
}
// lens are sorted descending: the number of entries > limit
__global__ void k_sweep_count_above(const uint32_t* __restrict__ len_desc, int n, uint32_t limit, unsigned int* __restrict__ out) {
  int lo = 0, hi = n;  // first index with len <= limit
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (len_desc[mid] > limit) lo = mid + 1; else hi = mid; }
  *out = (unsigned int)lo;
}
// slice of device column c: the last s with b[s] <= (position of c inside its owner's range)
__device__ __forceinline__ int sweep_slice_of(const SweepSlices& sl, int nslices, int c) {
  if (sl.nsub > 1) c -= (c / sl.stride) * sl.stride;
  int lo = 0, hi = nslices;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (sl.b[mid] <= c) lo = mid; else hi = mid; }
  return lo;
}
// the entry the sweep keeps for column c of slice `slice`: byte offset into the message vector, or (sharded form) GM_SWEEP_HOT | byte
// offset into the workgroup's LDS copy of the slice's busiest entries (graphmat_hip.h: gm_sweep_t.nsub)
__device__ __forceinline__ uint32_t sweep_entry_of(const SweepSlices& sl, int slice, int c) {
  if (sl.nsub <= 1) return (uint32_t)c << 2;
  const int q = c / sl.stride, j = c - q * sl.stride - sl.b[slice];
  const int slen = sl.b[slice + 1] - sl.b[slice], cap = sl.hot_words / sl.nsub;
  const int hq = slen < cap ? slen : cap;
  return j < hq ? (GM_SWEEP_HOT | ((uint32_t)(q * hq + j) << 2)) : ((uint32_t)c << 2);
}
// one wave per swept row (in length-rank order, the long rows first): its edges, keyed (set * 256 + workgroup, slice, slot), with
// the CSR position as the value; the row's edges keep their CSR order in the key stream (ranked offsets `off`)
__global__ void __launch_bounds__(kT)
k_sweep_keys(const int32_t* __restrict__ rows_ranked, int nswept, int nlong, int nsets, const unsigned long long* __restrict__ off,
             const int64_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, SweepSlices sl, int nslices, unsigned long long* __restrict__ key,
             uint32_t* __restrict__ val, int32_t* __restrict__ row_of_slot, int32_t* __restrict__ lrow_of_slot) {
  const int r = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
  if (r >= nswept) return;
  const int lane = threadIdx.x & 63;
  const int row = rows_ranked[r];
  const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
  const bool is_long = r < nlong;
  const unsigned q = (unsigned)(is_long ? r : r - nlong);
  const unsigned wg = q % 256u, l = q / 256u;
  const unsigned set = l % (unsigned)nsets, slot = l / (unsigned)nsets;
  const unsigned long long vw = (unsigned long long)set * 256ull + wg;
  if (lane == 0) {
    if (is_long) lrow_of_slot[vw * (unsigned long long)GM_SWEEP_LONG_SLOTS + slot] = row;
    else row_of_slot[vw * (unsigned long long)GM_SWEEP_ACC_ROWS + slot] = row;
  }
  const unsigned long long o = off[r];
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const int lo = sweep_slice_of(sl, nslices, colidx[e]);
    key[o + (unsigned long long)(e - e0)] = (vw << 23) | ((unsigned long long)lo << 16) | slot;
    val[o + (unsigned long long)(e - e0)] = (uint32_t)e;
  }
}
__global__ void __launch_bounds__(kT)
k_sweep_heads(const unsigned long long* __restrict__ key, int64_t n, uint32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i < n) head[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}
// pieces of the medium rows in (set, workgroup, slice, slot) order; rowmin[(set * 256 + w) * acc + slot] = the row's first slice
__global__ void __launch_bounds__(kT)
k_sweep_pieces(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ head, const uint32_t* __restrict__ pidx_incl, int64_t n,
               uint32_t* __restrict__ piece_start, uint16_t* __restrict__ piece_slot, uint32_t* __restrict__ piece_blk, int32_t* __restrict__ blk_first,
               int nslices, int* __restrict__ rowmin) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n || !head[i]) return;
  const uint32_t p = pidx_incl[i] - 1;
  const unsigned long long k = key[i];
  const unsigned slot = (unsigned)(k & 0xffffull), slice = (unsigned)((k >> 16) & 127ull);
  const unsigned long long vw = k >> 23;
  const uint32_t blk = (uint32_t)(vw * (unsigned long long)nslices + slice);
  piece_start[p] = (uint32_t)i;
  piece_slot[p] = (uint16_t)slot;
  piece_blk[p] = blk;
  if (i == 0 || (key[i - 1] >> 16) != (k >> 16)) blk_first[blk] = (int32_t)p;
  atomicMin(&rowmin[vw * (unsigned long long)GM_SWEEP_ACC_ROWS + slot], (int)slice);
}
// sort key of a piece inside its block: the longest first
__global__ void __launch_bounds__(kT)
k_sweep_piece_keys(const uint32_t* __restrict__ piece_start, const uint32_t* __restrict__ piece_blk, uint32_t np, unsigned long long* __restrict__ pkey,
                   uint32_t* __restrict__ pid) {
  const uint32_t p = blockIdx.x * kT + threadIdx.x;
  if (p >= np) return;
  const uint32_t len = piece_start[p + 1] - piece_start[p];
  pkey[p] = ((unsigned long long)piece_blk[p] << 16) | (unsigned long long)(0xffffu - (len > 0xffffu ? 0xffffu : len));
  pid[p] = p;
}
__global__ void __launch_bounds__(kT) k_sweep_block_groups(const int32_t* __restrict__ blk_first, int nblk, uint32_t* __restrict__ ng) {
  const int b = blockIdx.x * kT + threadIdx.x;
  if (b < nblk) ng[b] = (uint32_t)(blk_first[b + 1] - blk_first[b] + 63) / 64u;
}
// group g of block b = pieces q0 .. q0 + 63 of the block's sorted order; entries = 64 x its first (longest) piece
__global__ void __launch_bounds__(64)
k_sweep_group_sizes(const int32_t* __restrict__ blk_first, const uint32_t* __restrict__ grp_first, const uint32_t* __restrict__ sp,
                    const uint32_t* __restrict__ piece_start, unsigned long long* __restrict__ gsize, uint32_t* __restrict__ gq0, uint32_t* __restrict__ gblk,
                    const uint32_t* __restrict__ stream_first /* [nstream_blk + 1] first stream entry of the block, or null */, int nstream_blk) {
  const int b = blockIdx.x;
  const uint32_t g0 = grp_first[b], g1 = grp_first[b + 1];
  const uint32_t nm = (uint32_t)(blk_first[b + 1] - blk_first[b] + 63) / 64u;  // medium groups; behind them the block's stream groups
  for (uint32_t g = g0 + threadIdx.x; g < g1; g += 64) {
    if (g - g0 >= nm) {  // stream group j of the block: GM_STREAM_WIDTH rows of 64 of the block's short-row edges (the last one: what is left)
      const uint32_t j = g - g0 - nm;
      const uint32_t rows = (stream_first[b + 1] - stream_first[b] + 63u) / 64u;
      const uint32_t w = rows - j * GM_STREAM_WIDTH < GM_STREAM_WIDTH ? rows - j * GM_STREAM_WIDTH : GM_STREAM_WIDTH;
      gsize[g] = ((unsigned long long)w + 1ull) * 64ull;
      gq0[g] = j;
      gblk[g] = (uint32_t)b | 0x80000000u;
      continue;
    }
    const uint32_t q0 = (uint32_t)blk_first[b] + (g - g0) * 64u;
    const uint32_t p = sp[q0];
    gsize[g] = ((unsigned long long)(piece_start[p + 1] - piece_start[p]) + 1ull) * 64ull;  // (a meta row, then the longest piece's rows)
    gq0[g] = q0;
    gblk[g] = (uint32_t)b;
  }
}
__global__ void __launch_bounds__(kT) k_sweep_narrow(const unsigned long long* __restrict__ a, size_t n, uint32_t* __restrict__ o) {
  const size_t i = (size_t)blockIdx.x * kT + threadIdx.x;
  if (i < n) o[i] = (uint32_t)a[i];
}
// a group's entries: row 0 = the meta row (GM_SWEEP_PAD | width << 16 | first-piece flag << 15 | slot, slot 0x7fff: no piece),
// then transposed columns: scol[gbase + (1 + k) * 64 + lane] = byte offset of the k-th column of the lane's piece, or padding
__global__ void __launch_bounds__(kT)
k_sweep_fill(uint32_t ngroups, const uint32_t* __restrict__ gbase, const uint32_t* __restrict__ gq0, const uint32_t* __restrict__ gblk,
             const int32_t* __restrict__ blk_first, const uint32_t* __restrict__ sp, const uint32_t* __restrict__ piece_start,
             const uint16_t* __restrict__ piece_slot, const uint32_t* __restrict__ pos_sorted, const int32_t* __restrict__ colidx,
             const uint32_t* __restrict__ vals, SweepSlices sl, int nslices, const int* __restrict__ rowmin, uint32_t* __restrict__ scol,
             uint32_t* __restrict__ sval, uint32_t* __restrict__ src_pos) {
  for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    if (gblk[g] & 0x80000000u) continue;  // (a stream group: k_stream_fill)
    const uint32_t b = gblk[g], q0 = gq0[g], qe = (uint32_t)blk_first[b + 1];
    const uint32_t base = gbase[g], n = gbase[g + 1] - base;
    const uint32_t width = (n >> 6) - 1u;
    const uint32_t slice = b % (uint32_t)nslices, vw = b / (uint32_t)nslices;
    const uint32_t pad = sl.nsub > 1 ? (GM_SWEEP_PAD | GM_SWEEP_HOT) : (GM_SWEEP_PAD | ((uint32_t)sl.b[slice] << 2));
    const int lane = threadIdx.x & 63;
    const uint32_t q = q0 + lane;
    uint32_t ps = 0, len = 0;
    uint32_t meta = GM_SWEEP_PAD | (width << 16) | 0x7fffu;
    if (q < qe) {
      const uint32_t p = sp[q];
      ps = piece_start[p];
      len = piece_start[p + 1] - ps;
      const unsigned slot = piece_slot[p];
      const bool first = rowmin[(size_t)vw * GM_SWEEP_ACC_ROWS + slot] == (int)slice;
      meta = GM_SWEEP_PAD | (width << 16) | (first ? 0x8000u : 0u) | slot;
    }
    for (uint32_t j = threadIdx.x; j < n; j += kT) {
      uint32_t c = pad, v = 0u, sp_ = 0xffffffffu;
      if (j < 64) {
        c = meta;
      } else {
        const uint32_t k = (j >> 6) - 1u;
        if (k < len) {
          sp_ = pos_sorted[ps + k];
          c = sweep_entry_of(sl, (int)slice, colidx[sp_]);
          if (vals) v = vals[sp_];
        }
      }
      scol[base + j] = c;
      if (sval) sval[base + j] = v;
      if (src_pos) src_pos[base + j] = sp_;
    }
  }
}
// ---- the short rows as stream groups of the sweep (graphmat_hip.h: gm_sweep_t.nstream) ----
__global__ void __launch_bounds__(kT) k_stream_flag(const int64_t* __restrict__ rowptr, int nrows, int short_row, unsigned char* __restrict__ flag) {
  const int r = blockIdx.x * kT + threadIdx.x;
  if (r < nrows) { const int64_t l = rowptr[r + 1] - rowptr[r]; flag[r] = (l >= 1 && l <= short_row) ? 1 : 0; }
}
// one thread per short row (device order): its edges keyed (workgroup = bin % 256, slice, bin), value = the edge's index in the short rows'
// own CSR order (soff), spos[that index] = its position in the graph's CSR
__global__ void __launch_bounds__(kT)
k_stream_keys(const int32_t* __restrict__ srow, int nshort, const uint32_t* __restrict__ soff, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
              SweepSlices sl, int nslices, unsigned long long* __restrict__ key, uint32_t* __restrict__ val, uint32_t* __restrict__ spos) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= nshort) return;
  const int row = srow[i];
  const int64_t e0 = rowptr[row];
  const uint32_t o = soff[i], n = soff[i + 1] - o;
  const unsigned long long bin = o / (uint32_t)GM_STREAM_BIN, wg = bin & 255ull;
  for (uint32_t k = 0; k < n; k++) {
    const int lo = sweep_slice_of(sl, nslices, colidx[e0 + k]);
    key[o + k] = (wg << 31) | ((unsigned long long)lo << 24) | bin;
    val[o + k] = o + k;
    spos[o + k] = (uint32_t)(e0 + k);
  }
}
__device__ __forceinline__ uint32_t stream_lower_bound(const unsigned long long* __restrict__ key, uint32_t n, unsigned long long want) {
  uint32_t lo = 0, hi = n;  // first index with key >= want
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (key[mid] < want) lo = mid + 1; else hi = mid; }
  return lo;
}
// first[b] = first sorted entry of block b = workgroup * nslices + slice (first[nblk] = n); rows[b] = 64-entry rows the block's products take
__global__ void __launch_bounds__(kT)
k_stream_block_starts(const unsigned long long* __restrict__ key, uint32_t n, int nslices, int nblk, uint32_t* __restrict__ first) {
  const int b = blockIdx.x * kT + threadIdx.x;
  if (b > nblk) return;
  if (b == nblk) { first[b] = n; return; }
  const unsigned long long wg = (unsigned)b / (unsigned)nslices, sl = (unsigned)b % (unsigned)nslices;
  first[b] = stream_lower_bound(key, n, (wg << 31) | (sl << 24));
}
__global__ void __launch_bounds__(kT) k_stream_block_rows(const uint32_t* __restrict__ first, int nblk, uint32_t* __restrict__ rows, uint32_t* __restrict__ groups) {
  const int b = blockIdx.x * kT + threadIdx.x;
  if (b > nblk) return;
  const uint32_t r = b < nblk ? (first[b + 1] - first[b] + 63u) / 64u : 0u;
  rows[b] = r;
  groups[b] = (r + GM_STREAM_WIDTH - 1) / GM_STREAM_WIDTH;
}
__global__ void __launch_bounds__(kT) k_stream_add_groups(const uint32_t* __restrict__ groups, int nblk, uint32_t* __restrict__ ng) {
  const int b = blockIdx.x * kT + threadIdx.x;
  if (b < nblk) ng[b] += groups[b];
}
// schunk[(bin * nslices + slice) * 2] = where the bin's products of that slice start in the products stream, [.. + 1] = how many
__global__ void __launch_bounds__(kT)
k_stream_chunks(const unsigned long long* __restrict__ key, uint32_t n, int nslices, int nbins, const uint32_t* __restrict__ first, const uint32_t* __restrict__ row_base,
                uint32_t* __restrict__ schunk) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= (int64_t)nbins * nslices) return;
  const unsigned long long bin = (unsigned long long)(i / nslices), sl = (unsigned long long)(i % nslices), wg = bin & 255ull;
  const unsigned long long k0 = (wg << 31) | (sl << 24) | bin;
  const uint32_t lo = stream_lower_bound(key, n, k0), hi = stream_lower_bound(key, n, k0 + 1ull);
  const uint32_t b = (uint32_t)(wg * (unsigned long long)nslices + sl);
  schunk[i * 2] = row_base[b] * 64u + (lo - first[b]);
  schunk[i * 2 + 1] = hi - lo;
}
__global__ void __launch_bounds__(kT) k_stream_bin_rows(const uint32_t* __restrict__ soff, int nshort, int nbins, uint32_t* __restrict__ bin_row) {
  const int b = blockIdx.x * kT + threadIdx.x;
  if (b > nbins) return;
  if (b == nbins) { bin_row[b] = (uint32_t)nshort; return; }
  const uint32_t want = (uint32_t)b * (uint32_t)GM_STREAM_BIN;
  uint32_t lo = 0, hi = (uint32_t)nshort;  // first row with soff >= want
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (soff[mid] < want) lo = mid + 1; else hi = mid; }
  bin_row[b] = lo;
}
// the entries of the stream groups (k_sweep_fill skips them), and where each product belongs in its bin (sinv)
__global__ void __launch_bounds__(kT)
k_stream_fill(uint32_t ngroups, const uint32_t* __restrict__ gbase, const uint32_t* __restrict__ gq0, const uint32_t* __restrict__ gblk,
              const uint32_t* __restrict__ first, const uint32_t* __restrict__ row_base, const unsigned long long* __restrict__ key_sorted,
              const uint32_t* __restrict__ idx_sorted, const uint32_t* __restrict__ spos, const int32_t* __restrict__ colidx, const uint32_t* __restrict__ vals,
              SweepSlices sl, int nslices, uint32_t* __restrict__ scol, uint32_t* __restrict__ sval, uint32_t* __restrict__ src_pos, uint16_t* __restrict__ sinv) {
  for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    if (!(gblk[g] & 0x80000000u)) continue;
    const uint32_t b = gblk[g] & 0x7fffffffu, j = gq0[g];
    const uint32_t base = gbase[g], n = gbase[g + 1] - base, width = (n >> 6) - 1u;
    const uint32_t slice = b % (uint32_t)nslices;
    const uint32_t e_lo = first[b] + j * (GM_STREAM_WIDTH * 64u), e_end = first[b + 1];
    const uint32_t drow = row_base[b] + j * GM_STREAM_WIDTH;
    const uint32_t pad = sl.nsub > 1 ? (GM_SWEEP_PAD | GM_SWEEP_HOT) : (GM_SWEEP_PAD | ((uint32_t)sl.b[slice] << 2));
    for (uint32_t t = threadIdx.x; t < n; t += kT) {
      uint32_t c = pad, v = 0u, sp_ = 0xffffffffu;
      if (t < 64) {
        c = GM_SWEEP_PAD | 0x40000000u | (width << 16) | 0x7fffu | ((t < 32 && ((drow >> t) & 1u)) ? 0x8000u : 0u);
      } else {
        const uint32_t i = e_lo + (t - 64u);
        if (i < e_end) {
          const uint32_t k = idx_sorted[i];
          sp_ = spos[k];
          c = sweep_entry_of(sl, (int)slice, colidx[sp_]);
          if (vals) v = vals[sp_];
          const uint32_t bin = (uint32_t)(key_sorted[i] & 0xffffffull);
          sinv[(size_t)drow * 64 + (t - 64u)] = (uint16_t)(k - bin * (uint32_t)GM_STREAM_BIN);
        }
      }
      scol[base + t] = c;
      if (sval) sval[base + t] = v;
      if (src_pos) src_pos[base + t] = sp_;
    }
  }
}
// contiguous ranges of a block's groups for the 16 waves (wfirst: groups; wrow: 64-entry rows of scol), balanced by rows + 1 per group; the last waves (they fold the long
// rows of the block first: as many waves as the workgroup's long rows need lanes) get fold_share percent of an equal share
__global__ void __launch_bounds__(64)
k_sweep_wave_ranges(const uint32_t* __restrict__ grp_first, int nblk, const uint32_t* __restrict__ gbase, uint32_t* __restrict__ wfirst, uint32_t* __restrict__ wrow,
                    int fold_share, int fold_waves, int nwaves, const uint32_t* __restrict__ skip_groups /* per block: groups at its end to leave out, or null */,
                    int nskip_blk, const uint32_t* __restrict__ gblk = nullptr /* bit 31: a stream group */, int stream_weight = 100 /* percent of a medium row's cost */) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= nblk) return;
  constexpr int WS = 16;  // (entries per block in wfirst / wrow: WS + 1, whatever W)
  const int W = nwaves;
  const int FW = fold_waves;
  const uint32_t g0 = grp_first[b], g1 = grp_first[b + 1] - ((skip_groups != nullptr && b < nskip_blk) ? skip_groups[b] : 0u);
  // (a stream row is gathered like a medium row and its products are stored as well: its cost in medium rows = stream_weight percent)
  auto cost = [&](uint32_t g_) -> unsigned long long {
    const unsigned long long rows = (gbase[g_ + 1] - gbase[g_]) / 64u + 1u;
    return (gblk != nullptr && (gblk[g_] & 0x80000000u)) ? (rows * (unsigned)stream_weight + 99ull) / 100ull : rows;
  };
  unsigned long long total = 0;
  for (uint32_t g = g0; g < g1; g++) total += cost(g);
  const unsigned long long units = (unsigned long long)(W - FW) * 100ull + (unsigned long long)FW * (unsigned)fold_share;
  uint32_t g = g0;
  unsigned long long acc = 0, share = 0;
  for (int w = 0; w < W; w++) {
    wfirst[(size_t)b * (WS + 1) + w] = g;
    wrow[(size_t)b * (WS + 1) + w] = gbase[g] >> 6;
    share += w >= W - FW ? (unsigned)fold_share : 100u;
    const unsigned long long want = total * share / units;
    while (g < g1 && acc + (cost(g) + 1u) / 2u <= want) { acc += cost(g); g++; }
  }
  for (int w = W; w <= WS; w++) {  // (entry W ends the block; the entries behind it repeat the end)
    wfirst[(size_t)b * (WS + 1) + w] = g1;
    wrow[(size_t)b * (WS + 1) + w] = gbase[g1] >> 6;
  }
}
// long rows: entry e = ((set * 256 + w) * nslices + slice) * long_slots + j -> first position of that piece in the sorted keys
__global__ void __launch_bounds__(kT)
k_sweep_long_starts(const unsigned long long* __restrict__ key, int64_t n, int nslices, size_t nent, uint32_t* __restrict__ lps) {
  const size_t e = (size_t)blockIdx.x * kT + threadIdx.x;
  if (e > nent) return;
  if (e == nent) { lps[e] = (uint32_t)n; return; }
  const size_t b = e / GM_SWEEP_LONG_SLOTS;
  const unsigned long long vw = b / (size_t)nslices, slice = b % (size_t)nslices, j = e % GM_SWEEP_LONG_SLOTS;
  const unsigned long long want = (vw << 23) | (slice << 16) | j;
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (key[mid] >= want) hi = mid; else lo = mid + 1; }
  lps[e] = (uint32_t)lo;
}
__global__ void __launch_bounds__(kT)
k_sweep_long_fill(const unsigned long long* __restrict__ key_sorted, const uint32_t* __restrict__ pos_sorted, int64_t n, const int32_t* __restrict__ colidx,
                  const uint32_t* __restrict__ vals, SweepSlices sl, uint32_t* __restrict__ lcol, uint32_t* __restrict__ lval) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = pos_sorted[i];
  lcol[i] = sweep_entry_of(sl, (int)((key_sorted[i] >> 16) & 127ull), colidx[p]);
  if (lval) lval[i] = vals[p];
}
__global__ void __launch_bounds__(kT)
k_sweep_long_max(const uint32_t* __restrict__ lps, size_t nblk, unsigned int* __restrict__ out) {
  const size_t b = (size_t)blockIdx.x * kT + threadIdx.x;
  if (b < nblk) atomicMax(out, lps[(b + 1) * GM_SWEEP_LONG_SLOTS] - lps[b * GM_SWEEP_LONG_SLOTS]);
}
// The giant rows' edges for the sweep (gm_sweep_t.gcol / gdst): one wave per giant row writes, per edge, key = slice of its
// column, value = CSR position, and the edge's place in the products stream (gterm_off + position in the row); the stable
// sort by slice keeps (row, column) order inside a slice.
__global__ void __launch_bounds__(kT)
k_sweep_giant_keys(const int32_t* __restrict__ giant_row, int ngiant, const int64_t* __restrict__ gterm_off, const int64_t* __restrict__ rowptr,
                   const int32_t* __restrict__ colidx, SweepSlices sl, int nslices, uint8_t* __restrict__ key, uint32_t* __restrict__ pos,
                   uint32_t* __restrict__ dst) {
  const int gi = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
  if (gi >= ngiant) return;
  const int lane = threadIdx.x & 63;
  const int row = giant_row[gi];
  const int64_t e0 = rowptr[row], e1 = rowptr[row + 1], o = gterm_off[gi];
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const int lo = sweep_slice_of(sl, nslices, colidx[e]);
    key[o + (e - e0)] = (uint8_t)lo;
    pos[o + (e - e0)] = (uint32_t)e;
    dst[o + (e - e0)] = (uint32_t)(o + (e - e0));
  }
}
// (gterm_off is padded per row to multiples of 64: slots between rows carry key 255 and sort to the end)
__global__ void __launch_bounds__(kT)
k_sweep_giant_fill(const uint8_t* __restrict__ key_sorted, const uint32_t* __restrict__ pos_sorted, int64_t n, const int32_t* __restrict__ colidx,
                   const uint32_t* __restrict__ vals, SweepSlices sl, uint32_t* __restrict__ gcol, uint32_t* __restrict__ gval) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = pos_sorted[i];
  gcol[i] = sweep_entry_of(sl, (int)key_sorted[i], colidx[p]);
  if (gval) gval[i] = vals[p];
}

void free_sweep(gm_graph* g) {
  gm_sweep_t& S = g->sweep;
  const void* owned[] = {S.gcol, S.gval, S.gdst, S.gslice, S.gsrc_pos, S.scol, S.sval, S.gbase, S.wrow, S.wfirst, S.row_of_slot, S.lcol, S.lval, S.lps, S.lrow_of_slot, S.src_pos, S.lsrc_pos,
                         S.srow, S.soff, S.sbin_row, S.schunk, S.sinv, S.wrow_stream};
  for (const void* q : owned)
    if (q) (void)hipFree((void*)q);
  if (g->d_slice_base) (void)hipFree(g->d_slice_base);
  memset(&S, 0, sizeof(S));
  g->d_slice_base = nullptr;
}

// LDS words of the long rows' stage (the rest of the pool holds a slice's hot entries): the largest block in one round where that
// leaves most of the pool to the hot set
static int sweep_stage_words(int nrows_long, int max_long_block) {
  if (nrows_long <= 0) return 64;
  int stage = (max_long_block + 63) / 64 * 64;
  if (stage > GM_SWEEP_MAX_STAGE) stage = GM_SWEEP_MAX_STAGE;
  if (stage < 1024) stage = 1024;
  return stage;
}

// ---- what the stages hand each other -------------------------------------------------------------------------------------------

// A stage returns GM_OK, an error, or kNotSwept: this graph keeps its other passes, nothing more is built and build_sweep returns GM_OK.
constexpr int kNotSwept = -1;

struct SweepBuild {
  gm_graph* g;
  const CsrOwned* whole;
  hipStream_t s;
  int TS, nsub, nrows;  // slices; owners a slice spans (sharded: slice_base holds positions inside an owner's range); rows of this graph or shard
  const int64_t* rowptr;  // the whole-graph CSR
  const int32_t* colidx;
  const uint32_t* vals;  // (null: the adjacency keeps no edge values)
  SweepSlices sl;        // (hot_words is settled by the long rows' stage)
  // the options, read once
  int opt_long_row, acc_limit, long_limit, border_factor, fold_share, waves, stream, stream_weight;
  // counts, as the stages settle them
  uint32_t nswept = 0, nlong = 0, long_row = 0;  // swept rows; those above the medium / long border; the border (edges per row)
  int nsets = 0, per_wg_long = 0;                // launches; long rows per workgroup over all launches
  int64_t nedges_long = 0, nedges = 0;           // edges of the long rows / of the medium rows
  size_t nvw = 0, nblk = 0;                      // (launch, workgroup) pairs; blocks = pairs x slices
  int fold_waves() const { return std::min(8, (((per_wg_long + nsets - 1) / nsets) + 63) / 64); }  // waves of a block that fold its long rows first
};

// The swept rows' edges as (key, CSR position) pairs: [0, nedges_long) the long rows', behind them the medium rows', each part sorted
// by (set * 256 + workgroup, slice, slot).
struct SweptEdges {
  DevArray<u64> key;
  DevArray<uint32_t> pos;
  DevArray<int32_t> row_of_slot, lrow_of_slot;
};
struct LongRows {
  DevArray<uint32_t> lps, lcol, lval, lsrc_pos;
  unsigned int max_block = 0;
};
// The medium rows' pieces (a row's edges of one slice) and, per block, their order by descending length.
struct MediumPieces {
  uint32_t npieces = 0;
  DevArray<uint32_t> start;  // [npieces + 1] first sorted edge
  DevArray<uint16_t> slot;
  DevArray<int32_t> blk_first;  // [nblk + 1] first piece of the block
  DevArray<int> rowmin;         // first slice of every accumulator slot's row
  DevArray<uint32_t> sorted;    // piece ids, block by block, the longest first
  DevArray<uint32_t> ng;        // [nblk + 1] groups per block (the stream stage adds its own)
};
// The short rows as stream groups of the sweep (gm_sweep_t.nstream).
struct StreamGroups {
  bool built = false;
  uint32_t nshort = 0, edges = 0, rows_total = 0;
  int nbins = 0;
  DevArray<int32_t> srow;
  DevArray<uint32_t> soff, binrow, chunk;
  DevArray<uint16_t> inv;
  struct Scratch {  // what only the fill of the groups reads: dies with the medium stage
    DevArray<u64> keys;
    DevArray<uint32_t> idx, spos, first, rowbase, sgroups;
  };
};
struct MediumLayout {
  uint32_t ngroups = 0;
  u64 nentries = 0;
  DevArray<uint32_t> scol, sval, src_pos, gbase, wrow, wfirst, wrow_stream;
};
struct GiantEdges {
  int64_t nedges = 0;
  DevArray<uint32_t> gcol, gval, gdst, gslice, gsrc_pos;
};

// ---- the stages ----------------------------------------------------------------------------------------------------------------

// 1. The slices of the device order are reported even when no row ends up in the sweep (nrows = 0); then the early outs.
static int publish_slices(SweepBuild& c) {
  gm_graph* g = c.g;
  if (c.TS < 2 || c.TS > GM_MAX_SLICES) return kNotSwept;
  DevArray<int32_t> sb;
  int rc;
  if ((rc = sb.alloc(GM_MAX_SLICES + 2))) return rc;
  GM_TRY_HIP(hipMemcpyAsync(sb, g->slice_base, (size_t)(c.TS + 1) * 4, hipMemcpyHostToDevice, c.s));
  GM_TRY_HIP(hipStreamSynchronize(c.s));
  g->d_slice_base = sb.release();  // (owned by the graph from here on, swept or not: free_sweep)
  g->sweep.nslices = c.TS;
  g->sweep.slice_base = g->d_slice_base;
  const gm_csr_t& v = c.whole->view;
  if (c.nrows <= 0 || v.nnz >= ((int64_t)1 << 32) || g->desc.ndevice >= (c.nsub > 1 ? (1 << 28) : (1 << 29)) || (c.whole->vals != nullptr && v.val_bytes != 4)) return kNotSwept;
  return GM_OK;
}

// 2. The swept rows, ranked by length (descending; stable: ties by row id), so that the long rows come first.
static int rank_swept_rows(SweepBuild& c, DevArray<int32_t>& ranked, DevArray<uint32_t>& len_desc) {
  const gm_csr_t& v = c.whole->view;
  const int nrows = c.nrows;
  hipStream_t s = c.s;
  int rc;
  DevArray<int32_t> rows;
  {
    DevArray<unsigned char> flag;
    if ((rc = flag.alloc((size_t)nrows)) || (rc = rows.alloc((size_t)nrows))) return rc;
    GM_LAUNCH_1D(k_sweep_flag, nrows, s, c.rowptr, nrows, v.short_row, flag);
    // (giant rows keep their own passes -- k_giant_terms + the exact replay: a lane folding a 13 000-edge piece per slice would hold
    // its workgroup's slice barrier for the whole multiply)
    if (v.ngiant > 0) GM_LAUNCH_1D(k_sweep_unflag, v.ngiant, s, c.whole->giant_row, v.ngiant, flag);
    if ((rc = list_flagged(flag, nrows, rows.p, &c.nswept, s))) return rc;
  }
  if (c.nswept == 0) return kNotSwept;
  DevArray<uint32_t> len;
  if ((rc = len.alloc(c.nswept)) || (rc = len_desc.alloc(c.nswept)) || (rc = ranked.alloc(c.nswept))) return rc;
  GM_LAUNCH_1D(k_sweep_lens, c.nswept, s, rows, (int)c.nswept, c.rowptr, len);
  return radix_sort_pairs_desc(len.p, len_desc.p, rows.p, ranked.p, (size_t)c.nswept, 32, s);
}

// 3. The border between medium rows (64-wide groups) and long rows (staged through LDS, one lane folds a piece).  A piece is folded
// by ONE lane, row of entries after row: the longest medium piece of a slice is a chain that one wave has to walk while its
// workgroup's other waves wait at the slice barrier, so it should not exceed a wave's fair share of the block -- (medium
// entries per workgroup / 64) / 16 waves per slice, against ~L / nslices for a row of L edges: L <= medium edges / 262144 (phase
// clocks of the kernel, tools/sweep_lib_bench.hip: with the border at 4096 the slowest wave of an RMAT-26 workgroup spends
// 2.0 ms in its groups against 1.5 ms on average, at RMAT-24 1.2 against 0.33).  Candidates: powers of two from 256 to 4096;
// the long rows must fit their slots (long_slots per workgroup and launch) in as many launches as the medium rows need.
// hl: the swept rows' lengths, descending.
static uint32_t choose_long_border(const std::vector<uint32_t>& hl, int acc_limit, int long_limit, int border_factor) {
  const size_t nswept = hl.size();
  // for a border L, the long rows are the prefix with len > L
  auto rows_above = [&](uint32_t L) { size_t lo = 0, hi = nswept; while (lo < hi) { const size_t mid = (lo + hi) / 2; if (hl[mid] > L) lo = mid + 1; else hi = mid; } return lo; };
  std::vector<u64> suffix(nswept + 1, 0ull);  // edges of the rows from position i on
  for (size_t i = nswept; i-- > 0;) suffix[i] = suffix[i + 1] + hl[i];
  // launches a border needs: the medium rows must fit the accumulator slots, the long rows theirs
  auto sets_for = [&](uint32_t L) {
    const size_t nl = rows_above(L), nm = nswept - nl;
    const size_t a = ((nm + 255) / 256 + (size_t)acc_limit - 1) / (size_t)acc_limit, b = ((nl + 255) / 256 + (size_t)long_limit - 1) / (size_t)long_limit;
    return std::max<size_t>(1, std::max(a, b));
  };
  size_t fewest = ~(size_t)0;
  for (uint32_t L = 4096; L >= 256; L >>= 1) fewest = std::min(fewest, sets_for(L));
  uint32_t smallest_ok = 4096;
  for (uint32_t L = 4096; L >= 256; L >>= 1) {
    if (sets_for(L) != fewest) continue;
    smallest_ok = L;
    const u64 emed = suffix[rows_above(L)];
    if ((u64)L * 262144ull <= emed * (u64)border_factor) return L;
  }
  return smallest_ok;
}
// ... the border (forced by gm_set_option("sweep_long_row"), else chosen), the rows above it, and the launches both kinds need
static int split_at_border(SweepBuild& c, const DevArray<uint32_t>& len_desc) {
  hipStream_t s = c.s;
  int rc;
  if (c.opt_long_row > 0) {
    c.long_row = (uint32_t)std::min(c.opt_long_row, 8191);  // (13 bits for a group's width)
  } else {
    std::vector<uint32_t> hl(c.nswept);
    if ((rc = read_back(hl.data(), len_desc.p, s, c.nswept))) return rc;
    c.long_row = choose_long_border(hl, c.acc_limit, c.long_limit, c.border_factor);
  }
  DevArray<unsigned int> cnt;
  if ((rc = cnt.alloc(4))) return rc;
  hipLaunchKernelGGL(k_sweep_count_above, dim3(1), dim3(1), 0, s, len_desc, (int)c.nswept, c.long_row, cnt);
  if ((rc = read_back(&c.nlong, cnt.p, s))) return rc;
  const unsigned int nmed = c.nswept - c.nlong;
  const int per_wg_med = (int)((nmed + 255u) / 256u);
  c.per_wg_long = (int)((c.nlong + 255u) / 256u);
  c.nsets = std::max(1, std::max((per_wg_med + c.acc_limit - 1) / c.acc_limit, (c.per_wg_long + c.long_limit - 1) / c.long_limit));
  if (c.nsets > 16) return kNotSwept;  // (12 key bits for set * 256 + workgroup)
  c.nvw = (size_t)c.nsets * 256;
  c.nblk = c.nvw * (size_t)c.TS;
  return GM_OK;
}

// 4. The edge offsets of the ranked rows, a key per edge, and the two stable sorts: inside (set, workgroup, slice, slot) the edges keep
// their ascending native column order.  Takes over the ranked list and its lengths: nothing behind this stage reads them.
static int sort_swept_edges(SweepBuild& c, DevArray<int32_t> ranked, DevArray<uint32_t> len_desc, SweptEdges& e) {
  hipStream_t s = c.s;
  const size_t nswept = c.nswept;
  int rc;
  DevArray<u64> l64, off;
  if ((rc = l64.alloc(nswept + 1)) || (rc = off.alloc(nswept + 1))) return rc;
  GM_TRY_HIP(l64.fill(0, nswept + 1, s));
  GM_LAUNCH_1D(k_sweep_widen, nswept, s, len_desc, (int)nswept, l64);
  if ((rc = exclusive_scan(l64.p, off.p, nswept + 1, s))) return rc;
  u64 tot_edges = 0, long_edges = 0;
  GM_TRY_HIP(hipMemcpyAsync(&tot_edges, off + nswept, 8, hipMemcpyDeviceToHost, s));
  if ((rc = read_back(&long_edges, off.p + c.nlong, s))) return rc;
  const int64_t nedges_all = (int64_t)tot_edges;
  c.nedges_long = (int64_t)long_edges;
  c.nedges = nedges_all - c.nedges_long;
  if (nedges_all <= 0 || nedges_all >= ((int64_t)1 << 32)) return kNotSwept;
  DevArray<u64> k_in;
  DevArray<uint32_t> v_in;
  if ((rc = k_in.alloc((size_t)nedges_all)) || (rc = e.key.alloc((size_t)nedges_all)) || (rc = v_in.alloc((size_t)nedges_all)) || (rc = e.pos.alloc((size_t)nedges_all)) ||
      (rc = e.row_of_slot.alloc(c.nvw * GM_SWEEP_ACC_ROWS)) || (rc = e.lrow_of_slot.alloc(c.nvw * GM_SWEEP_LONG_SLOTS)))
    return rc;
  GM_TRY_HIP(e.row_of_slot.fill(0xff, c.nvw * GM_SWEEP_ACC_ROWS, s));
  GM_TRY_HIP(e.lrow_of_slot.fill(0xff, c.nvw * GM_SWEEP_LONG_SLOTS, s));
  hipLaunchKernelGGL(k_sweep_keys, dim3((c.nswept + (kT / 64) - 1) / (kT / 64)), dim3(kT), 0, s, ranked, (int)c.nswept, (int)c.nlong, c.nsets, off,
                     c.rowptr, c.colidx, c.sl, c.TS, k_in, v_in, e.row_of_slot, e.lrow_of_slot);
  GM_TRY_HIP(hipGetLastError());
  const unsigned key_bits = 23u + (unsigned)bits_for((uint32_t)c.nvw);
  if (c.nedges_long > 0 && (rc = radix_sort_pairs(k_in.p, e.key.p, v_in.p, e.pos.p, (size_t)c.nedges_long, key_bits, s))) return rc;
  if (c.nedges > 0 && (rc = radix_sort_pairs(k_in.p + c.nedges_long, e.key.p + c.nedges_long, v_in.p + c.nedges_long, e.pos.p + c.nedges_long, (size_t)c.nedges, key_bits, s))) return rc;
  GM_TRY_HIP(hipStreamSynchronize(s));
  return GM_OK;
}

// 5. The long rows: where every (block, slot) piece starts, the entries, the largest block -- and with it the stage the kernel needs,
// which fixes how many words of the LDS pool are left for a slice's hot entries (c.sl.hot_words).
static int build_long_rows(SweepBuild& c, const SweptEdges& e, LongRows& L) {
  hipStream_t s = c.s;
  const size_t nent = c.nblk * GM_SWEEP_LONG_SLOTS;
  const int64_t nl = c.nedges_long;
  int rc;
  DevArray<unsigned int> cnt;
  if ((rc = L.lps.alloc(nent + 1)) || (rc = L.lcol.alloc((size_t)nl + 64)) || (rc = cnt.alloc(4))) return rc;
  if (c.vals && (rc = L.lval.alloc((size_t)nl + 64))) return rc;
  GM_LAUNCH_1D(k_sweep_long_starts, nent + 1, s, e.key, nl, c.TS, nent, L.lps);
  GM_TRY_HIP(cnt.fill(0, 1, s));
  GM_LAUNCH_1D(k_sweep_long_max, c.nblk, s, L.lps, c.nblk, cnt);
  if ((rc = read_back(&L.max_block, cnt.p, s))) return rc;
  // the LDS pool is shared by a slice's hot entries and the long rows' stage (engine.hpp: multiply_out_swept chooses the same stage)
  c.sl.hot_words = GM_SWEEP_POOL - sweep_stage_words((int)c.nlong, (int)L.max_block);
  if (nl > 0) GM_LAUNCH_1D(k_sweep_long_fill, nl, s, e.key, e.pos, nl, c.colidx, c.vals, c.sl, L.lcol, L.lval);
  if (c.vals && nl > 0) {  // (with edge values: the entries' CSR positions stay, for gm_graph_sync_tile_vals)
    if ((rc = L.lsrc_pos.alloc((size_t)nl))) return rc;
    GM_TRY_HIP(hipMemcpyAsync(L.lsrc_pos, e.pos, (size_t)nl * 4, hipMemcpyDeviceToDevice, s));
  }
  GM_TRY_HIP(hipStreamSynchronize(s));
  return GM_OK;
}

// 6a. The medium rows: their pieces in (set, workgroup, slice, slot) order, every block's pieces by descending length, and how many
// groups of 64 pieces of similar length each block gets.
static int cut_medium_pieces(const SweepBuild& c, const SweptEdges& e, MediumPieces& P) {
  hipStream_t s = c.s;
  const int64_t nedges = c.nedges;
  const size_t nblk = c.nblk;
  const u64* mkey = e.key + c.nedges_long;
  int rc;
  DevArray<uint32_t> pblk;
  {
    DevArray<uint32_t> head, pidx;
    if ((rc = head.alloc((size_t)nedges)) || (rc = pidx.alloc((size_t)nedges))) return rc;
    GM_LAUNCH_1D(k_sweep_heads, nedges, s, mkey, nedges, head);
    if ((rc = inclusive_scan(head.p, pidx.p, (size_t)nedges, s)) || (rc = read_back(&P.npieces, pidx.p + (nedges - 1), s))) return rc;
    const size_t np = P.npieces;
    if ((rc = P.start.alloc(np + 1)) || (rc = P.slot.alloc(np + 1)) || (rc = pblk.alloc(np + 1)) || (rc = P.blk_first.alloc(nblk + 1)) ||
        (rc = P.rowmin.alloc(c.nvw * GM_SWEEP_ACC_ROWS)))
      return rc;
    GM_TRY_HIP(P.blk_first.fill(0xff, nblk + 1, s));
    GM_TRY_HIP(P.rowmin.fill(0x7f, c.nvw * GM_SWEEP_ACC_ROWS, s));
    GM_LAUNCH_1D(k_sweep_pieces, nedges, s, mkey, head, pidx, nedges, P.start, P.slot, pblk, P.blk_first, c.TS, P.rowmin);
    const uint32_t ne32 = (uint32_t)nedges;
    GM_TRY_HIP(hipMemcpyAsync(P.start + np, &ne32, 4, hipMemcpyHostToDevice, s));
    // a block without pieces starts where the next one does
    std::vector<int32_t> h(nblk + 1);
    if ((rc = read_back(h.data(), P.blk_first.p, s, nblk + 1))) return rc;
    h[nblk] = (int32_t)np;
    for (int64_t b = (int64_t)nblk - 1; b >= 0; b--) if (h[b] < 0) h[b] = h[b + 1];
    GM_TRY_HIP(hipMemcpyAsync(P.blk_first, h.data(), (nblk + 1) * 4, hipMemcpyHostToDevice, s));
    GM_TRY_HIP(hipStreamSynchronize(s));
  }
  {  // the pieces of a block, longest first (stable: equal lengths keep their slot order)
    const size_t np = P.npieces;
    DevArray<u64> pk_in, pk_out;
    DevArray<uint32_t> pid_in;
    if ((rc = pk_in.alloc(np)) || (rc = pk_out.alloc(np)) || (rc = pid_in.alloc(np)) || (rc = P.sorted.alloc(np))) return rc;
    GM_LAUNCH_1D(k_sweep_piece_keys, np, s, P.start, pblk, P.npieces, pk_in, pid_in);
    if ((rc = radix_sort_pairs(pk_in.p, pk_out.p, pid_in.p, P.sorted.p, np, 16u + (unsigned)bits_for((uint32_t)nblk), s))) return rc;
    GM_TRY_HIP(hipStreamSynchronize(s));
  }
  if ((rc = P.ng.alloc(nblk + 1))) return rc;
  GM_TRY_HIP(P.ng.fill(0, nblk + 1, s));
  GM_LAUNCH_1D(k_sweep_block_groups, nblk, s, P.blk_first, (int)nblk, P.ng);
  return GM_OK;
}

// 7. The short rows (1 .. short_row edges) as STREAM groups behind the medium groups of the first launch's blocks (gm_sweep_t.nstream):
// listed in device order, cut into bins of ~GM_STREAM_BIN edges, bin b -> workgroup b % 256; their edges sorted (workgroup, slice, bin, row,
// column) -- stable, so a row's edges keep their ascending native column order inside every (bin, slice) chunk.  Adds every block's
// stream groups to ng.
// (shards too: the entries carry the build-time hot-set decision like every other entry of a sharded structure)
static int build_stream_groups(const SweepBuild& c, uint32_t* ng, StreamGroups& st, StreamGroups::Scratch& tmp) {
  hipStream_t s = c.s;
  const int nrows = c.nrows, TS = c.TS, nsblk = 256 * TS;
  int rc;
  {
    DevArray<unsigned char> flag;
    if ((rc = flag.alloc((size_t)nrows)) || (rc = st.srow.alloc((size_t)nrows + 1))) return rc;
    GM_LAUNCH_1D(k_stream_flag, nrows, s, c.rowptr, nrows, c.whole->view.short_row, flag);
    if ((rc = list_flagged(flag, nrows, st.srow.p, &st.nshort, s))) return rc;
  }
  if (st.nshort > 0) {
    DevArray<uint32_t> len;
    if ((rc = len.alloc((size_t)st.nshort + 1)) || (rc = st.soff.alloc((size_t)st.nshort + 1))) return rc;
    GM_TRY_HIP(len.fill(0, (size_t)st.nshort + 1, s));
    GM_LAUNCH_1D(k_sweep_lens, st.nshort, s, st.srow, (int)st.nshort, c.rowptr, len);
    if ((rc = exclusive_scan(len.p, st.soff.p, (size_t)st.nshort + 1, s)) || (rc = read_back(&st.edges, st.soff.p + st.nshort, s))) return rc;
  }
  st.nbins = (int)(((u64)st.edges + GM_STREAM_BIN - 1) / GM_STREAM_BIN);
  if (st.edges == 0 || st.nbins >= (1 << 24)) return GM_OK;
  {
    DevArray<u64> kin;
    DevArray<uint32_t> vin;
    if ((rc = kin.alloc(st.edges)) || (rc = tmp.keys.alloc(st.edges)) || (rc = vin.alloc(st.edges)) || (rc = tmp.idx.alloc(st.edges)) || (rc = tmp.spos.alloc(st.edges))) return rc;
    GM_LAUNCH_1D(k_stream_keys, st.nshort, s, st.srow, (int)st.nshort, st.soff, c.rowptr, c.colidx, c.sl, TS, kin, vin, tmp.spos);
    GM_TRY_HIP(hipGetLastError());
    if ((rc = radix_sort_pairs(kin.p, tmp.keys.p, vin.p, tmp.idx.p, (size_t)st.edges, 39, s))) return rc;
    GM_TRY_HIP(hipStreamSynchronize(s));
  }
  DevArray<uint32_t> rows;  // 64-entry rows of every block's products
  if ((rc = tmp.first.alloc((size_t)nsblk + 2)) || (rc = rows.alloc((size_t)nsblk + 2)) || (rc = tmp.sgroups.alloc((size_t)nsblk + 2)) || (rc = tmp.rowbase.alloc((size_t)nsblk + 2)) ||
      (rc = st.binrow.alloc((size_t)st.nbins + 2)) || (rc = st.chunk.alloc((size_t)st.nbins * TS * 2 + 16)))
    return rc;
  GM_LAUNCH_1D(k_stream_block_starts, nsblk + 1, s, tmp.keys, st.edges, TS, nsblk, tmp.first);
  GM_LAUNCH_1D(k_stream_block_rows, nsblk + 1, s, tmp.first, nsblk, rows, tmp.sgroups);
  if ((rc = exclusive_scan(rows.p, tmp.rowbase.p, (size_t)nsblk + 1, s))) return rc;
  GM_TRY_HIP(hipMemcpyAsync(&st.rows_total, tmp.rowbase + nsblk, 4, hipMemcpyDeviceToHost, s));
  GM_LAUNCH_1D(k_stream_add_groups, nsblk, s, tmp.sgroups, nsblk, ng);
  GM_LAUNCH_1D(k_stream_bin_rows, st.nbins + 1, s, st.soff, (int)st.nshort, st.nbins, st.binrow);
  GM_LAUNCH_1D(k_stream_chunks, (int64_t)st.nbins * TS, s, tmp.keys, st.edges, TS, st.nbins, tmp.first, tmp.rowbase, st.chunk);
  GM_TRY_HIP(hipGetLastError());
  GM_TRY_HIP(hipStreamSynchronize(s));
  if ((rc = st.inv.alloc((size_t)st.rows_total * 64 + 32))) return rc;
  GM_TRY_HIP(st.inv.fill(0xff, (size_t)st.rows_total * 64 + 32, s));
  st.built = true;
  return GM_OK;
}

// 6b. The groups of all blocks (medium groups, behind them the block's stream groups), their transposed entries, and contiguous
// ranges of every block's groups for its waves -- without the stream groups (wrow) and, when there are any, with them (wrow_stream:
// the kernel form that stores their products walks these).
static int fill_groups(const SweepBuild& c, const SweptEdges& e, const MediumPieces& P, const StreamGroups& st, const StreamGroups::Scratch& tmp, MediumLayout& M) {
  hipStream_t s = c.s;
  const size_t nblk = c.nblk;
  const uint32_t* mpos = e.pos + c.nedges_long;
  int rc;
  DevArray<uint32_t> grp_first, gq0, gblk;
  if ((rc = grp_first.alloc(nblk + 1)) || (rc = exclusive_scan(P.ng.p, grp_first.p, nblk + 1, s)) || (rc = read_back(&M.ngroups, grp_first.p + nblk, s))) return rc;
  const size_t ng1 = (size_t)M.ngroups + 1;
  {
    DevArray<u64> gsize, gb64;
    if ((rc = gsize.alloc(ng1)) || (rc = gb64.alloc(ng1)) || (rc = gq0.alloc(ng1)) || (rc = gblk.alloc(ng1)) || (rc = M.gbase.alloc(ng1))) return rc;
    GM_TRY_HIP(gsize.fill(0, ng1, s));
    hipLaunchKernelGGL(k_sweep_group_sizes, dim3((unsigned)nblk), dim3(64), 0, s, P.blk_first, grp_first, P.sorted,
                       P.start, gsize, gq0, gblk, st.built ? tmp.first : nullptr, 256 * c.TS);
    if ((rc = exclusive_scan(gsize.p, gb64.p, ng1, s)) || (rc = read_back(&M.nentries, gb64.p + M.ngroups, s))) return rc;
    if (M.nentries >= (1ull << 32)) return kNotSwept;  // (32-bit entry positions; the graph keeps its tile passes)
    GM_LAUNCH_1D(k_sweep_narrow, ng1, s, gb64, ng1, M.gbase);
  }
  const size_t nentries = (size_t)M.nentries;
  if ((rc = M.scol.alloc(nentries + 64 * 64)) || (rc = M.wrow.alloc(nblk * 17)) || (rc = M.wfirst.alloc(nblk * 17))) return rc;
  if (c.vals && ((rc = M.sval.alloc(nentries + 64 * 64)) || (rc = M.src_pos.alloc(nentries + 64)))) return rc;
  hipLaunchKernelGGL(k_sweep_fill, dim3(65536), dim3(kT), 0, s, M.ngroups, M.gbase, gq0, gblk, P.blk_first,
                     P.sorted, P.start, P.slot, mpos, c.colidx, c.vals, c.sl, c.TS, P.rowmin, M.scol, M.sval, M.src_pos);
  if (st.built)
    hipLaunchKernelGGL(k_stream_fill, dim3(65536), dim3(kT), 0, s, M.ngroups, M.gbase, gq0, gblk, tmp.first,
                       tmp.rowbase, tmp.keys, tmp.idx, tmp.spos, c.colidx, c.vals, c.sl, c.TS, M.scol, M.sval, M.src_pos,
                       st.inv);
  const dim3 wgrid((unsigned)((nblk + 63) / 64));
  const int fold_share = c.nlong > 0 ? c.fold_share : 100;
  hipLaunchKernelGGL(k_sweep_wave_ranges, wgrid, dim3(64), 0, s, grp_first, (int)nblk, M.gbase, M.wfirst, M.wrow, fold_share, c.fold_waves(), c.waves,
                     st.built ? tmp.sgroups : nullptr, 256 * c.TS);
  DevArray<uint32_t> wfirst_stream;
  if (st.built) {
    if ((rc = M.wrow_stream.alloc(nblk * 17)) || (rc = wfirst_stream.alloc(nblk * 17))) return rc;
    hipLaunchKernelGGL(k_sweep_wave_ranges, wgrid, dim3(64), 0, s, grp_first, (int)nblk, M.gbase, wfirst_stream, M.wrow_stream, fold_share, c.fold_waves(),
                       16, nullptr, 0, gblk, c.stream_weight);
  }
  GM_TRY_HIP(hipGetLastError());
  GM_TRY_HIP(hipStreamSynchronize(s));
  return GM_OK;
}

// 8. No medium row: empty blocks for every wave.
// (the kernel requests a wave's first batch of entries -- and their values -- before it knows that the stream is empty: both arrays exist)
static int empty_groups(const SweepBuild& c, MediumLayout& M) {
  hipStream_t s = c.s;
  int rc;
  if ((rc = M.gbase.alloc(16)) || (rc = M.wrow.alloc(c.nblk * 17)) || (rc = M.wfirst.alloc(c.nblk * 17)) || (rc = M.scol.alloc(64 * 64))) return rc;
  GM_TRY_HIP(M.scol.fill(0xff, 64 * 64, s));
  if (c.vals) {
    if ((rc = M.sval.alloc(64 * 64))) return rc;
    GM_TRY_HIP(M.sval.fill(0, 64 * 64, s));
  }
  GM_TRY_HIP(M.gbase.fill(0, 16, s));
  GM_TRY_HIP(M.wfirst.fill(0, c.nblk * 17, s));
  GM_TRY_HIP(M.wrow.fill(0, c.nblk * 17, s));
  GM_TRY_HIP(hipStreamSynchronize(s));
  return GM_OK;
}

// 9. The giant rows' edges by slice: the sweep gathers their messages with its hot sets and writes the products where the giant
// rows' fold passes expect them (gterm_off), so those passes need not gather at all.
static int giant_edges_by_slice(const SweepBuild& c, GiantEdges& G) {
  const gm_csr_t& v = c.whole->view;
  if (v.ngiant <= 0 || v.giant_edges <= 0 || v.giant_edges >= ((int64_t)1 << 32)) return GM_OK;
  hipStream_t s = c.s;
  const size_t ge = (size_t)v.giant_edges;  // (slots, rows padded to multiples of 64)
  int rc;
  DevArray<uint8_t> k_in, k_out;
  DevArray<uint32_t> p_in, p_out, d_in;
  if ((rc = k_in.alloc(ge)) || (rc = k_out.alloc(ge)) || (rc = p_in.alloc(ge)) || (rc = p_out.alloc(ge)) || (rc = d_in.alloc(ge)) || (rc = G.gdst.alloc(ge)) ||
      (rc = G.gslice.alloc(GM_MAX_SLICES + 2)))
    return rc;
  GM_TRY_HIP(k_in.fill(0xff, ge, s));
  GM_TRY_HIP(p_in.fill(0, ge, s));
  GM_TRY_HIP(d_in.fill(0, ge, s));
  hipLaunchKernelGGL(k_sweep_giant_keys, dim3((v.ngiant + (kT / 64) - 1) / (kT / 64)), dim3(kT), 0, s, c.whole->giant_row, v.ngiant, c.whole->gterm_off,
                     c.rowptr, c.colidx, c.sl, c.TS, k_in, p_in, d_in);
  // two stable sorts by the same keys: positions and destinations travel together
  if ((rc = radix_sort_pairs(k_in.p, k_out.p, p_in.p, p_out.p, ge, 8, s)) || (rc = radix_sort_pairs(k_in.p, k_out.p, d_in.p, G.gdst.p, ge, 8, s))) return rc;
  hipLaunchKernelGGL(k_key_bounds<uint32_t>, dim3(1), dim3(256), 0, s, k_out, (int64_t)ge, c.TS, G.gslice);
  uint32_t nreal = 0;
  if ((rc = read_back(&nreal, G.gslice.p + c.TS, s))) return rc;
  G.nedges = (int64_t)nreal;
  if ((rc = G.gcol.alloc((size_t)nreal + 64))) return rc;
  if (c.vals && (rc = G.gval.alloc((size_t)nreal + 64))) return rc;
  if (nreal > 0) GM_LAUNCH_1D(k_sweep_giant_fill, nreal, s, k_out, p_out, (int64_t)nreal, c.colidx, c.vals, c.sl, G.gcol, G.gval);
  GM_TRY_HIP(hipGetLastError());
  GM_TRY_HIP(hipStreamSynchronize(s));
  if (c.vals) G.gsrc_pos = std::move(p_out);  // (with edge values: the CSR positions stay, for gm_graph_sync_tile_vals)
  return GM_OK;
}

// 10. Everything is built: the graph takes the arrays over.
static void publish_sweep(const SweepBuild& c, SweptEdges& e, LongRows& L, MediumLayout& M, StreamGroups& st, GiantEdges& G) {
  gm_sweep_t& S = c.g->sweep;
  S.ngiant_edges = G.nedges;
  S.gcol = G.gcol.release(); S.gval = G.gval.release(); S.gdst = G.gdst.release(); S.gslice = G.gslice.release(); S.gsrc_pos = G.gsrc_pos.release();
  S.nrows = (int32_t)c.nswept; S.nrows_long = (int32_t)c.nlong; S.nsets = c.nsets; S.nslices = c.TS;
  S.acc_rows = GM_SWEEP_ACC_ROWS; S.long_slots = GM_SWEEP_LONG_SLOTS; S.max_long_block = (int32_t)L.max_block; S.val_bytes = c.vals ? 4 : 0;
  S.short_row = c.whole->view.short_row; S.long_row = (int32_t)c.long_row;
  S.nedges = c.nedges; S.nedges_long = c.nedges_long; S.nentries = (int64_t)M.nentries; S.ngroups = (int64_t)M.ngroups;
  S.scol = M.scol.release(); S.sval = M.sval.release(); S.gbase = M.gbase.release(); S.wrow = M.wrow.release(); S.wfirst = M.wfirst.release();
  S.src_pos = M.src_pos.release();
  S.row_of_slot = e.row_of_slot.release(); S.lrow_of_slot = e.lrow_of_slot.release();
  S.lcol = L.lcol.release(); S.lval = L.lval.release(); S.lps = L.lps.release(); S.lsrc_pos = L.lsrc_pos.release();
  S.slice_base = c.g->d_slice_base;
  S.nsub = c.nsub; S.stride = c.sl.stride; S.hot_words = c.sl.hot_words;
  S.waves = c.waves;
  if (st.built) {
    S.nstream = (int64_t)st.edges; S.nstream_slots = (int64_t)st.rows_total * 64; S.nshort_rows = (int32_t)st.nshort; S.nbins = st.nbins;
    S.bin_cap = GM_STREAM_BIN; S.stream_width = GM_STREAM_WIDTH;
    S.srow = st.srow.release(); S.soff = st.soff.release(); S.sbin_row = st.binrow.release(); S.schunk = st.chunk.release(); S.sinv = st.inv.release();
    S.wrow_stream = M.wrow_stream.release();
  }
}

int build_sweep(gm_graph* g, const CsrOwned* whole, hipStream_t s) {
  memset(&g->sweep, 0, sizeof(g->sweep));
  SweepBuild c;
  c.g = g; c.whole = whole; c.s = s;
  c.TS = g->nslices;
  c.nsub = g->desc.nshards > 1 ? g->desc.nshards : 1;
  c.nrows = g->desc.row_hi - g->desc.row_lo;
  c.rowptr = whole->rowptr; c.colidx = whole->colidx; c.vals = (const uint32_t*)whole->vals;
  memset(&c.sl, 0, sizeof(c.sl));
  for (int t = 0; t <= c.TS && t < GM_MAX_SLICES + 2; t++) c.sl.b[t] = g->slice_base[t];
  c.sl.nsub = c.nsub;
  c.sl.stride = c.nsub > 1 ? c.nrows : 0;
  c.sl.hot_words = GM_SWEEP_POOL - 64;  // (settled by build_long_rows, once the long rows' largest block -- the stage it needs -- is known)
  c.opt_long_row = g_sweep_long_row; c.acc_limit = g_sweep_acc_limit; c.long_limit = g_sweep_long_limit; c.border_factor = g_sweep_border_factor;
  c.fold_share = g_sweep_fold_share; c.waves = (g_sweep_waves == 12 || g_sweep_waves == 8) ? g_sweep_waves : 16;
  c.stream = g_sweep_stream; c.stream_weight = g_sweep_stream_weight;
#define GM_STAGE(call) do { const int rc_ = (call); if (rc_ != GM_OK) return rc_ == kNotSwept ? GM_OK : rc_; } while (0)
  DevArray<int32_t> ranked;
  DevArray<uint32_t> len_desc;
  SweptEdges edges;
  LongRows lng;
  StreamGroups stream;
  MediumLayout med;
  GiantEdges giant;
  GM_STAGE(publish_slices(c));
  GM_STAGE(rank_swept_rows(c, ranked, len_desc));
  GM_STAGE(split_at_border(c, len_desc));
  GM_STAGE(sort_swept_edges(c, std::move(ranked), std::move(len_desc), edges));
  GM_STAGE(build_long_rows(c, edges, lng));
  if (c.nedges > 0) {
    MediumPieces pieces;
    StreamGroups::Scratch stream_tmp;
    GM_STAGE(cut_medium_pieces(c, edges, pieces));
    if (c.stream != 0) GM_STAGE(build_stream_groups(c, pieces.ng, stream, stream_tmp));
    GM_STAGE(fill_groups(c, edges, pieces, stream, stream_tmp, med));
  } else {
    GM_STAGE(empty_groups(c, med));
  }
  GM_STAGE(giant_edges_by_slice(c, giant));
  publish_sweep(c, edges, lng, med, stream, giant);
#undef GM_STAGE
  return GM_OK;
}

}  // namespace gm
