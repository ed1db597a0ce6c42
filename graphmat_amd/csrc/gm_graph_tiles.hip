// gm_graph_tiles.hip -- column tiles of the GM_DIR_OUT adjacency (graphmat_hip.h: gm_graph_tile): one CSR per tile from the whole
// graph's sorted keys; a tiled graph then gets its sweep and its blocked stream (gm_graph_sweep.hip, gm_graph_blocked.hip).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "gm_build.hpp"

namespace gm {

// tile of a device id: the last t with base[t] <= d
__device__ __forceinline__ int tile_of_dev(int d, const int32_t* __restrict__ base, int ntiles) {
  int t = 0;
  while (t + 1 < ntiles && base[t + 1] <= d) t++;
  return t;
}
// tile of every sorted edge: the tile whose device-id range holds its column; 255 = not tiled (short row)
struct TileBases { int32_t b[GM_MAX_TILES + 1]; };
__global__ void __launch_bounds__(kT)
k_tile_keys(const uint64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ rowptr, int short_row,
            const int32_t* __restrict__ dev_of_native, TileBases bases, int ntiles, uint8_t* __restrict__ tkey, uint32_t* __restrict__ pos) {
  const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (k >= n) return;
  const uint64_t key = keys[k];
  const int row = (int)(key >> 32);
  const int cn = (int)(uint32_t)key;
  const bool tiled = rowptr[row + 1] - rowptr[row] > short_row;
  tkey[k] = tiled ? (uint8_t)tile_of_dev(dev_of_native[cn], bases.b, ntiles) : (uint8_t)255;
  pos[k] = (uint32_t)k;
}
__global__ void __launch_bounds__(kT)
k_tile_gather(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ pos, int64_t n,
              uint64_t* __restrict__ keys_t, uint32_t* __restrict__ idx_t) {
  const int64_t j = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (j >= n) return;
  const uint32_t p = pos[j];
  keys_t[j] = keys[p];
  idx_t[j] = idx[p];
}
// rows of more than `limit` edges in the whole graph (column tiles with row classes fixed per row)
__global__ void __launch_bounds__(kT)
k_own_wave_rows(const int64_t* __restrict__ rowptr, int nrows, int64_t limit, unsigned char* __restrict__ flag) {
  int r = blockIdx.x * kT + threadIdx.x;
  if (r < nrows) flag[r] = (rowptr[r + 1] - rowptr[r] > limit) ? 1 : 0;
}

// The sorted edges' positions grouped by tile (stable: inside a tile the edges keep their (row, native col) order);
// h_bounds[t] = where tile t starts in pos_by_tile
static int sort_edges_by_tile(gm_graph* g, const uint64_t* keys_sorted, unsigned long long kept, const CsrOwned* whole, hipStream_t s, DevArray<uint32_t>& pos_by_tile,
                              std::vector<int64_t>& h_bounds) {
  const int T = g->ntiles;
  int rc;
  DevArray<uint8_t> tk_in, tk_out;
  DevArray<uint32_t> pos_in;
  DevArray<int64_t> bounds;
  if ((rc = tk_in.alloc((size_t)kept)) || (rc = tk_out.alloc((size_t)kept)) || (rc = pos_in.alloc((size_t)kept)) || (rc = pos_by_tile.alloc((size_t)kept)) ||
      (rc = bounds.alloc((size_t)GM_MAX_TILES + 2)))
    return rc;
  if (kept == 0) return GM_OK;
  TileBases bases;
  memcpy(bases.b, g->tile_base, sizeof(bases.b));
  GM_LAUNCH_1D(k_tile_keys, kept, s, keys_sorted, (int64_t)kept, whole->rowptr, whole->view.tile_min_row, g->dev_of_native, bases, T, tk_in, pos_in);
  GM_TRY_HIP(hipGetLastError());
  if ((rc = radix_sort_pairs(tk_in.p, tk_out.p, pos_in.p, pos_by_tile.p, (size_t)kept, 8, s))) return rc;
  hipLaunchKernelGGL(k_key_bounds<int64_t>, dim3(1), dim3(128), 0, s, tk_out, (int64_t)kept, T, bounds);
  return read_back(h_bounds.data(), bounds.p, s, (size_t)T + 1);
}

int build_tiles(gm_graph* g, const uint64_t* keys_sorted, const uint32_t* idx_sorted, unsigned long long kept, const void* d_val, hipStream_t s, const CsrOwned* whole) {
  const int T = g->ntiles;
  const int nrows = g->desc.row_hi - g->desc.row_lo;
  const int nw = (nrows + 31) / 32 + 2;
  int rc;
  g->out_tiles = new CsrOwned[T];
  g->out_tile_prev = new uint32_t*[T];
  for (int t = 0; t < T; t++) g->out_tile_prev[t] = nullptr;
  DevArray<uint32_t> pos_by_tile;
  std::vector<int64_t> h_bounds((size_t)T + 1, 0);
  if ((rc = sort_edges_by_tile(g, keys_sorted, kept, whole, s, pos_by_tile, h_bounds))) return rc;
  int64_t largest = 0;
  for (int t = 0; t < T; t++) largest = std::max(largest, h_bounds[t + 1] - h_bounds[t]);
  DevArray<uint64_t> keys_t;
  DevArray<uint32_t> idx_t;
  if ((rc = keys_t.alloc((size_t)largest)) || (rc = idx_t.alloc((size_t)largest))) return rc;
  // Row classes fixed per row (g_own_wave_row > 0): a row of more than that many edges in the WHOLE graph is worked on
  // by the one-wave-per-row / giant kernels in every tile, all other rows by the row-block / 16-row kernels in every
  // tile -- the two groups then never touch the same y entry, and the engine can run them on two streams through all
  // tiles of an iteration without joining them after every tile.
  DevArray<unsigned char> own_wave;
  int own_limit = g_own_wave_row;
  if (own_limit == 0) { const char* e = getenv("GRAPHMAT_OWN_WAVE_ROW"); if (e) own_limit = atoi(e); }
  if (own_limit > 0 && nrows > 0) {
    if ((rc = own_wave.alloc((size_t)nrows))) return rc;
    GM_LAUNCH_1D(k_own_wave_rows, nrows, s, whole->rowptr, nrows, (int64_t)own_limit, own_wave);
  }
  uint32_t* prev = nullptr;
  GM_TRY_HIP(hipMalloc((void**)&prev, (size_t)nw * 4));
  GM_TRY_HIP(hipMemsetAsync(prev, 0, (size_t)nw * 4, s));
  g->out_tile_prev[0] = prev;
  for (int t = 0; t < T; t++) {
    const int64_t n = h_bounds[t + 1] - h_bounds[t];
    if (n > 0) GM_LAUNCH_1D(k_tile_gather, n, s, keys_sorted, idx_sorted, pos_by_tile + h_bounds[t], n, keys_t, idx_t);
    if ((rc = finish_csr(g, keys_t, idx_t, (unsigned long long)n, d_val, s, &g->out_tiles[t], -1, own_wave))) return rc;
    gm_csr_t& v = g->out_tiles[t].view;
    v.hot_base = g->tile_base[t];
    v.hot_len = g->tile_base[t + 1] - g->tile_base[t];
    if (t + 1 < T) {  // presence bits of the rows with an edge in an earlier tile
      uint32_t* nxt = nullptr;
      GM_TRY_HIP(hipMalloc((void**)&nxt, (size_t)nw * 4));
      GM_LAUNCH_1D(k_or_words<uint32_t>, nw, s, g->out_tile_prev[t], g->out_tiles[t].rowbits, nxt, nw);
      g->out_tile_prev[t + 1] = nxt;
    }
  }
  GM_TRY_HIP(hipStreamSynchronize(s));
  if (g_sweep_slices != 0 && (rc = build_sweep(g, whole, s))) return rc;
  if (g_sweep_slices != 0 && (rc = build_blocked(g, whole, s))) return rc;
  return GM_OK;
}

void free_tiles(gm_graph* g) {
  free_sweep(g);
  free_blocked(g);
  if (g->out_tiles) {
    for (int t = 0; t < g->ntiles; t++) free_csr(&g->out_tiles[t]);
    delete[] g->out_tiles;
    g->out_tiles = nullptr;
  }
  if (g->out_tile_prev) {
    for (int t = 0; t < g->ntiles; t++)
      if (g->out_tile_prev[t]) (void)hipFree(g->out_tile_prev[t]);
    delete[] g->out_tile_prev;
    g->out_tile_prev = nullptr;
  }
}

}  // namespace gm
