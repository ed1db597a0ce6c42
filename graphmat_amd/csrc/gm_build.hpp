// gm_build.hpp -- shared by the translation units that build a graph's layouts:
//   gm_graph.hip          key sort, CSR and row classes, the device order, the graph's lifetime, the C-ABI
//   gm_graph_tiles.hip    column tiles            (gm_graph_tile)
//   gm_graph_sweep.hip    row-stationary sweep    (gm_sweep_t)
//   gm_graph_blocked.hip  column-blocked stream   (gm_blocked_t)
// Typed device buffers, the rocprim two-call idiom in one place, scalar read-back, the layout options and the entry points
// the units call across files.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <type_traits>

#include "gm_internal.hpp"

namespace gm {

// ---- layout options (gm_set_option / gm_reset_options in gm_programs.hip; defined, with what they mean, in gm_graph.hip) ----
extern int g_short_row, g_giant_row, g_rank_cap, g_rank_by, g_tile_min_row, g_tile_balance, g_long_mid, g_sort_tile_lists, g_own_wave_row, g_col_tiles;
extern int g_sweep_slices, g_sweep_border_factor, g_sweep_stream_weight, g_sweep_stream, g_sweep_waves, g_sweep_fold_share, g_sweep_long_row, g_sweep_acc_limit,
    g_sweep_long_limit;
extern int g_blocked_rows;

constexpr int kT = 256;
inline int grid_for(int64_t n) { return (int)((n + kT - 1) / kT); }
// one thread per item, kT threads per workgroup
#define GM_LAUNCH_1D(kernel, n, stream, ...) hipLaunchKernelGGL(kernel, dim3(gm::grid_for((int64_t)(n))), dim3(gm::kT), 0, stream, __VA_ARGS__)

inline int bits_for(uint32_t maxval) {
  int b = 0;
  while ((1ull << b) <= (uint64_t)maxval) b++;
  return b;
}

// A device array that frees itself.  Sizes are in elements; it converts to T* wherever a kernel or a copy wants one.
// (hipFree waits for the device, so an array may go out of scope while work that reads it is still queued.)
template <class T>
struct DevArray {
  T* p = nullptr;
  DevArray() = default;
  DevArray(const DevArray&) = delete;
  DevArray& operator=(const DevArray&) = delete;
  DevArray(DevArray&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevArray& operator=(DevArray&& o) noexcept {
    if (this != &o) { free(); p = o.p; o.p = nullptr; }
    return *this;
  }
  ~DevArray() { free(); }
  int alloc(size_t n) {
    free();
    size_t bytes = n * sizeof(T);
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc((void**)&p, bytes);
    if (e != hipSuccess) { set_error("hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); p = nullptr; return GM_ERR_NOMEM; }
    return GM_OK;
  }
  void free() { if (p) { (void)hipFree(p); p = nullptr; } }
  hipError_t fill(int byte, size_t n, hipStream_t s) { return hipMemsetAsync(p, byte, n * sizeof(T), s); }
  operator T*() const { return p; }
  T* release() { T* q = p; p = nullptr; return q; }
};
using DevBuf = DevArray<unsigned char>;  // bytes: edge values of any width, rocprim's temporary storage

// h[0, n) <- d[0, n), and wait for it
template <class T>
inline int read_back(T* h, const typename std::common_type<T>::type* d /* (not deduced: a DevArray<T> converts) */, hipStream_t s, size_t n = 1) {
  GM_TRY_HIP(hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, s));
  GM_TRY_HIP(hipStreamSynchronize(s));
  return GM_OK;
}

// ---- rocprim: ask for the temporary size, allocate, call again -- spelled out here and nowhere else.  The wrappers below
// queue their work on `s` and do not wait for it.  Each owns its temporary storage (releasing it waits for the device) unless the
// caller lends one: calls queued back to back then share it, grown when too small, and nothing waits between them.
struct RocTemp { DevBuf buf; size_t bytes = 0; };
template <class Call>
inline int with_rocprim_temp(Call&& call, RocTemp* lent = nullptr) {
  RocTemp own;
  RocTemp& t = lent ? *lent : own;
  size_t tb = 0;
  int rc;
  GM_TRY_HIP(call((void*)nullptr, tb));
  if (t.bytes < tb + 256) {
    if ((rc = t.buf.alloc(tb + 256))) return rc;
    t.bytes = tb + 256;
  }
  GM_TRY_HIP(call((void*)t.buf.p, tb));
  return GM_OK;
}
// out <- the items of in[0, n) whose flag is set, in order; *d_count <- how many
template <class In, class Out>
inline int select(In in, const unsigned char* flags, Out out, unsigned int* d_count, size_t n, hipStream_t s, RocTemp* lent = nullptr) {
  return with_rocprim_temp([&](void* t, size_t& tb) { return rocprim::select(t, tb, in, flags, out, d_count, n, s); }, lent);
}
// stable sorts of (key, value) pairs by bits [0, end_bit) of the key
template <class K, class V>
int radix_sort_pairs(const K* kin, K* kout, const V* vin, V* vout, size_t n, unsigned end_bit, hipStream_t s) {
  return with_rocprim_temp([&](void* t, size_t& tb) { return rocprim::radix_sort_pairs(t, tb, kin, kout, vin, vout, n, 0u, end_bit, s); });
}
template <class K, class V>
int radix_sort_pairs_desc(const K* kin, K* kout, const V* vin, V* vout, size_t n, unsigned end_bit, hipStream_t s) {
  return with_rocprim_temp([&](void* t, size_t& tb) { return rocprim::radix_sort_pairs_desc(t, tb, kin, kout, vin, vout, n, 0u, end_bit, s); });
}
// (a radix sort is megabytes of device code per key / value type: those that several units use are compiled once, in gm_graph_sweep.hip)
extern template int radix_sort_pairs_desc<uint32_t, int32_t>(const uint32_t*, uint32_t*, const int32_t*, int32_t*, size_t, unsigned, hipStream_t);
extern template int radix_sort_pairs<unsigned long long, uint32_t>(const unsigned long long*, unsigned long long*, const uint32_t*, uint32_t*, size_t, unsigned, hipStream_t);
extern template int radix_sort_pairs<uint8_t, uint32_t>(const uint8_t*, uint8_t*, const uint32_t*, uint32_t*, size_t, unsigned, hipStream_t);
template <class X>
inline int exclusive_scan(const X* in, X* out, size_t n, hipStream_t s) {
  return with_rocprim_temp([&](void* t, size_t& tb) { return rocprim::exclusive_scan(t, tb, in, out, X(0), n, rocprim::plus<X>(), s); });
}
template <class X>
inline int inclusive_scan(const X* in, X* out, size_t n, hipStream_t s) {
  return with_rocprim_temp([&](void* t, size_t& tb) { return rocprim::inclusive_scan(t, tb, in, out, n, rocprim::plus<X>(), s); });
}

// ---- kernels more than one unit launches (templates: a unit that does not launch one does not carry it) ----
template <class T>
__global__ void __launch_bounds__(kT) k_fill_iota(T* __restrict__ a, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i < n) a[i] = (T)i;
}
// out[t] = first position of the sorted 8-bit keys whose key is >= t (t in [0, nkeys]); one workgroup of more than nkeys threads
template <class Out>
__global__ void k_key_bounds(const uint8_t* __restrict__ key_sorted, int64_t n, int nkeys, Out* __restrict__ out) {
  const int t = threadIdx.x;
  if (t > nkeys) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int)key_sorted[mid] < t) lo = mid + 1; else hi = mid;
  }
  out[t] = (Out)lo;
}
template <class W>
__global__ void __launch_bounds__(kT) k_or_words(const W* __restrict__ a, const W* __restrict__ b, W* __restrict__ o, int n) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i < n) o[i] = a[i] | b[i];
}

// rows[0, *count) <- the i < n whose flag is set, ascending (the row lists of the sweep, its stream groups and the blocked stream)
// (a template like the kernels above: only the units that call it carry its kernels)
template <class Row>
inline int list_flagged(const unsigned char* flag, int n, Row* rows, unsigned int* count, hipStream_t s) {
  DevArray<Row> iota;
  DevArray<unsigned int> cnt;
  int rc;
  if ((rc = iota.alloc((size_t)n)) || (rc = cnt.alloc(4))) return rc;
  GM_LAUNCH_1D(k_fill_iota<Row>, n, s, iota, n);
  if ((rc = select(iota.p, flag, rows, cnt, (size_t)n, s))) return rc;
  return read_back(count, cnt, s);
}

// the slices of the device order as a kernel argument (sweep and blocked stream)
struct SweepSlices { int32_t b[GM_MAX_SLICES + 2]; int32_t nsub, stride, hot_words, pad_; };

// ---- entry points across the units ----
// gm_graph.hip
int finish_csr(gm_graph* g, const uint64_t* keys_sorted, const uint32_t* idx_sorted, unsigned long long kept, const void* d_val, hipStream_t s, CsrOwned* out,
               int tile_split = -1, const unsigned char* own_wave = nullptr);
void free_csr(CsrOwned* c);
// gm_graph_tiles.hip (build_tiles goes on to build the sweep and the blocked stream of a tiled graph; free_tiles frees those too)
int build_tiles(gm_graph* g, const uint64_t* keys_sorted, const uint32_t* idx_sorted, unsigned long long kept, const void* d_val, hipStream_t s,
                const CsrOwned* whole);
void free_tiles(gm_graph* g);
// gm_graph_sweep.hip
int build_sweep(gm_graph* g, const CsrOwned* whole, hipStream_t s);
void free_sweep(gm_graph* g);
// gm_graph_blocked.hip
int build_blocked(gm_graph* g, const CsrOwned* whole, hipStream_t s);
void free_blocked(gm_graph* g);

}  // namespace gm
