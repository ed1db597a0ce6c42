// gm_graph_blocked.hip -- builds gm_blocked_t: the short rows of a graph without skew as a column-blocked stream
// (graphmat_hip.h: gm_blocked_t; kernels.hpp: k_spmv_blocked)
#include <string.h>

#include <vector>

#include "gm_build.hpp"

namespace gm {

using u64 = unsigned long long;

int g_blocked_rows = 0;  // 0: automatic, 1: whenever the graph has slices, -1: never (gm_set_option("blocked_rows"))

__global__ void __launch_bounds__(kT) k_blocked_flag(const int64_t* __restrict__ rowptr, int nrows, int short_row, unsigned char* __restrict__ flag) {
  const int r = blockIdx.x * kT + threadIdx.x;
  if (r < nrows) { const int64_t l = rowptr[r + 1] - rowptr[r]; flag[r] = (l >= 1 && l <= short_row) ? 1 : 0; }
}
// The short rows are dealt over the blocks in runs of 64 consecutive rows (run j -> block j % nblk): the device order is degree-ranked inside
// a slice, so blocks of CONSECUTIVE rows would hold up to twice as many entries at the top of a slice as at its bottom -- and workgroups
// that walk the slices in step wait for the heaviest block of the pass (measured on the uniform 2^26 graph: 14.3 ms against 11 for the
// prototype's equal blocks).  A run's results are 256 contiguous bytes of y.
__global__ void __launch_bounds__(kT) k_blocked_deal(const int32_t* __restrict__ rows, int ns, int nblk, int32_t* __restrict__ dealt) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= ns) return;
  const int j = i >> 6;
  dealt[(size_t)(j % nblk) * GM_BLOCKED_ROWS + (size_t)(j / nblk) * 64 + (i & 63)] = rows[i];
}
// (slots: the blocks' row slots, -1 = no row)
__global__ void __launch_bounds__(kT) k_blocked_lens(const int32_t* __restrict__ slots, int n, const int64_t* __restrict__ rowptr, unsigned long long* __restrict__ len) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i < n) len[i] = slots[i] >= 0 ? (unsigned long long)(rowptr[slots[i] + 1] - rowptr[slots[i]]) : 0ull;
}
// key = block | slice (7 bits) | row slot inside the block (15 bits); value = the edge's position in the CSR
__global__ void __launch_bounds__(kT)
k_blocked_keys(const int32_t* __restrict__ slots, int n, const unsigned long long* __restrict__ off, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
               SweepSlices sl, int TS, unsigned long long* __restrict__ key, uint32_t* __restrict__ pos) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const int r = slots[i];
  if (r < 0) return;
  const int64_t a = rowptr[r], e = rowptr[r + 1];
  const unsigned long long hi = ((unsigned long long)(i / GM_BLOCKED_ROWS) << 22), lo = (unsigned long long)(i % GM_BLOCKED_ROWS);
  unsigned long long o = off[i];
  for (int64_t k = a; k < e; k++, o++) {
    const int c = colidx[k];
    int s0 = 0, s1 = TS;  // slice of column c: sl.b[s] <= c < sl.b[s + 1]
    while (s1 - s0 > 1) { const int mid = (s0 + s1) / 2; if (sl.b[mid] <= c) s0 = mid; else s1 = mid; }
    key[o] = hi | ((unsigned long long)s0 << 15) | lo;
    pos[o] = (uint32_t)k;
  }
}
__global__ void __launch_bounds__(kT)
k_blocked_fill(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ pos, int64_t n, const int32_t* __restrict__ slots, const int64_t* __restrict__ rowptr,
               const int32_t* __restrict__ colidx, const uint32_t* __restrict__ vals, int TS, uint32_t* __restrict__ ecol, uint16_t* __restrict__ erow,
               uint32_t* __restrict__ eval, uint32_t* __restrict__ toff) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = key[i];
  const uint32_t local = (uint32_t)(k & 0x7fffu), slice = (uint32_t)(k >> 15) & 127u;
  const size_t blk = (size_t)(k >> 22);
  const int r = slots[blk * GM_BLOCKED_ROWS + local];
  const uint32_t p = pos[i];
  ecol[i] = (uint32_t)colidx[p];
  if (eval) eval[i] = vals[p];
  erow[i] = (uint16_t)(local | ((int64_t)p == rowptr[r] ? 0x8000u : 0u));
  if (i == 0 || (key[i - 1] >> 15) != (k >> 15)) toff[blk * (size_t)TS + slice] = (uint32_t)i;
}
// where the 16 waves of a workgroup start inside a (block, slice) segment: equal shares, moved forward to the next row border
__global__ void __launch_bounds__(kT) k_blocked_wave_offsets(const uint32_t* __restrict__ toff, const uint16_t* __restrict__ erow, size_t nseg, uint32_t* __restrict__ woff) {
  const size_t t = (size_t)blockIdx.x * kT + threadIdx.x;
  if (t >= nseg * 17) return;
  const size_t seg = t / 17;
  const int w = (int)(t % 17);
  const uint32_t a = toff[seg], e = toff[seg + 1];
  uint32_t p = w == 16 ? e : a + (uint32_t)(((unsigned long long)(e - a) * (unsigned)w) / 16u);
  while (p > a && p < e && (erow[p] & 0x7fffu) == (erow[p - 1] & 0x7fffu)) p++;
  woff[t] = p;
}

void free_blocked(gm_graph* g) {
  gm_blocked_t& B = g->blocked;
  const void* owned[] = {B.ecol, B.erow, B.woff, B.row_of, B.step_count, B.eval, B.epos};
  for (const void* q : owned)
    if (q) (void)hipFree((void*)q);
  memset(&B, 0, sizeof(B));
}

// The short rows in device order, dealt over the blocks' row slots (-1 = no row); *ns = how many there are (0: none, nothing dealt)
static int deal_short_rows(const CsrOwned* whole, int nrows, hipStream_t s, unsigned int* ns, int* nblk, DevArray<int32_t>& dealt) {
  int rc;
  DevArray<unsigned char> flag;
  DevArray<int32_t> rows;
  if ((rc = flag.alloc((size_t)nrows)) || (rc = rows.alloc((size_t)nrows))) return rc;
  GM_LAUNCH_1D(k_blocked_flag, nrows, s, whole->rowptr, nrows, whole->view.short_row, flag);
  if ((rc = list_flagged(flag, nrows, rows.p, ns, s))) return rc;
  *nblk = (int)(((size_t)*ns + GM_BLOCKED_ROWS - 1) / GM_BLOCKED_ROWS);
  if (*ns == 0 || *nblk >= (1 << 16)) return GM_OK;
  const size_t nslots = (size_t)*nblk * GM_BLOCKED_ROWS;
  if ((rc = dealt.alloc(nslots))) return rc;
  GM_TRY_HIP(dealt.fill(0xff, nslots, s));
  GM_LAUNCH_1D(k_blocked_deal, *ns, s, rows, (int)*ns, *nblk, dealt);
  GM_TRY_HIP(hipStreamSynchronize(s));
  return GM_OK;
}

int build_blocked(gm_graph* g, const CsrOwned* whole, hipStream_t s) {
  memset(&g->blocked, 0, sizeof(g->blocked));
  const int TS = g->nslices;
  const int nrows = g->desc.row_hi - g->desc.row_lo;
  if (g_blocked_rows < 0 || TS < 2 || TS > GM_MAX_SLICES || nrows <= 0 || (whole->vals != nullptr && whole->view.val_bytes != 4) || whole->view.nnz <= 0 || whole->view.nnz >= ((int64_t)1 << 32) - 65536 ||
      g->desc.nshards > 1 || whole->view.short_row <= 0 || whole->view.short_row > 16384)
    return GM_OK;
  if (g_blocked_rows == 0 && (double)g->nlive * 4.0 < 48.0 * 1048576.0) return GM_OK;
  const int64_t* rowptr = whole->rowptr;
  const int32_t* colidx = whole->colidx;
  const uint32_t* vals = (const uint32_t*)whole->vals;
  int rc;
  unsigned int ns = 0;
  int nblk = 0;
  DevArray<int32_t> dealt;
  if ((rc = deal_short_rows(whole, nrows, s, &ns, &nblk, dealt))) return rc;
  if (ns == 0 || nblk >= (1 << 16)) return GM_OK;
  const int nslots = nblk * GM_BLOCKED_ROWS;
  // the entries: a key per edge, sorted by (block, slice, row slot)
  int64_t nent = 0;
  DevArray<u64> k_out;
  DevArray<uint32_t> v_out;
  {
    DevArray<u64> off;
    {
      DevArray<u64> l64;
      if ((rc = l64.alloc((size_t)nslots + 1)) || (rc = off.alloc((size_t)nslots + 1))) return rc;
      GM_TRY_HIP(l64.fill(0, (size_t)nslots + 1, s));
      GM_LAUNCH_1D(k_blocked_lens, nslots, s, dealt, nslots, rowptr, l64);
      u64 tot = 0;
      if ((rc = exclusive_scan(l64.p, off.p, (size_t)nslots + 1, s)) || (rc = read_back(&tot, off.p + nslots, s))) return rc;
      nent = (int64_t)tot;
    }
    // automatic: a graph without skew -- (nearly) every edge in a short row; with hot vertices the row-blocks and the sweep are faster
    // (profiles/r05_short_rows_blocked_stream_prototype.md: RMAT-26's short rows 2.8-3.2 ms this way against 1.27-1.30)
    if (nent <= 0 || (g_blocked_rows == 0 && (double)nent < 0.9 * (double)whole->view.nnz)) return GM_OK;
    DevArray<u64> k_in;
    DevArray<uint32_t> v_in;
    if ((rc = k_in.alloc((size_t)nent)) || (rc = k_out.alloc((size_t)nent)) || (rc = v_in.alloc((size_t)nent)) || (rc = v_out.alloc((size_t)nent))) return rc;
    SweepSlices sl;
    memset(&sl, 0, sizeof(sl));
    for (int t = 0; t <= TS; t++) sl.b[t] = g->slice_base[t];
    GM_LAUNCH_1D(k_blocked_keys, nslots, s, dealt, nslots, off, rowptr, colidx, sl, TS, k_in, v_in);
    GM_TRY_HIP(hipGetLastError());
    // stable: inside a (block, slice, row) the edges keep their CSR order = ascending native column
    if ((rc = radix_sort_pairs(k_in.p, k_out.p, v_in.p, v_out.p, (size_t)nent, 22u + (unsigned)bits_for((uint32_t)nblk), s))) return rc;
    GM_TRY_HIP(hipStreamSynchronize(s));
  }
  const size_t nseg = (size_t)nblk * TS, npad = (size_t)nent + 64 * 64;
  const int npass = (nblk + 255) / 256;
  const int nsteps = npass * TS;
  DevArray<uint32_t> ecol, toff, woff, steps, eval;
  DevArray<uint16_t> erow;
  if (vals && (rc = eval.alloc(npad))) return rc;
  if (vals) GM_TRY_HIP(eval.fill(0, npad, s));
  if ((rc = ecol.alloc(npad)) || (rc = erow.alloc(npad)) || (rc = toff.alloc(nseg + 2)) || (rc = woff.alloc((nseg + 1) * 17)) || (rc = steps.alloc((size_t)8 * nsteps + 64))) return rc;
  GM_TRY_HIP(ecol.fill(0, npad, s));
  GM_TRY_HIP(erow.fill(0, npad, s));
  GM_TRY_HIP(toff.fill(0xff, nseg + 2, s));
  GM_TRY_HIP(steps.fill(0, (size_t)8 * nsteps + 64, s));
  GM_LAUNCH_1D(k_blocked_fill, nent, s, k_out, v_out, nent, dealt, rowptr, colidx, vals, TS, ecol, erow, eval, toff);
  GM_TRY_HIP(hipGetLastError());
  {  // a (block, slice) segment without entries starts where the next one does
    std::vector<uint32_t> h(nseg + 1);
    if ((rc = read_back(h.data(), toff.p, s, nseg))) return rc;
    h[nseg] = (uint32_t)nent;
    for (size_t b = nseg; b-- > 0;) if (h[b] == 0xffffffffu) h[b] = h[b + 1];
    GM_TRY_HIP(hipMemcpyAsync(toff, h.data(), (nseg + 1) * 4, hipMemcpyHostToDevice, s));
    GM_TRY_HIP(hipStreamSynchronize(s));
  }
  hipLaunchKernelGGL(k_blocked_wave_offsets, dim3((unsigned)((nseg * 17 + kT - 1) / kT)), dim3(kT), 0, s, toff, erow, nseg, woff);
  GM_TRY_HIP(hipGetLastError());
  GM_TRY_HIP(hipStreamSynchronize(s));
  gm_blocked_t& B = g->blocked;
  B.nrows = (int32_t)ns; B.nblocks = nblk; B.nslices = TS; B.short_row = whole->view.short_row; B.nsteps = nsteps; B.nentries = nent;
  B.ecol = ecol.release(); B.erow = erow.release(); B.woff = woff.release(); B.row_of = dealt.release(); B.step_count = steps.release();
  B.val_bytes = vals ? 4 : 0; B.eval = eval.release();
  B.epos = vals ? v_out.release() : nullptr;  // (with edge values: the entries' CSR positions stay, for gm_graph_sync_tile_vals)
  return GM_OK;
}

}  // namespace gm
