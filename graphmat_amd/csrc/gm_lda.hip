// gm_lda.hip -- LDA topic modelling (the semantics of the reference's src/LDA.cpp), K = 20, fp64.
//
// A corpus is a bipartite graph: documents are vertices 1..ndoc, words the next nterms, an edge document -> word
// carries a token count.  Every vertex holds K topic counts N[0..K).  Three vertex programs:
//   init    every edge draws K pseudo-random shares of its count (glibc's rand_r seeded with the count), a vertex's N is
//           the sum over its edges;
//   step    every edge redistributes its count over the topics in proportion to
//           (N_dst + a - 1) * (N_src + b - 1) / (global_N + vocab * (eta - 1)), a vertex's new N is the sum over its
//           edges (both directions); global_N, the sum of N over the word vertices, is recomputed after every iteration;
//   loglik  every word sums count * log(phi . theta) over its edges.
// Each exists twice, computing the same bits:
//   * as an ordinary GraphMat::GraphProgram (LdaInitP / LdaP / LdaLLP) run by the common engine through run_fixed --
//     option "force_ordered" selects this form;
//   * as dedicated kernels in the shape of the wide SGD kernels of gm_programs.hip (the default): the messages as compact
//     160-byte rows, one wave per row, a tile of edges at a time, phase A lane = edge (the per-edge arithmetic, in place in
//     the LDS tile), phase B lane = component (the ordered fold over the tile's edges).
// The per-edge arithmetic is the same __host__ __device__ functions in both forms (and in gm_lda_edge_init).
// Built with -ffp-contract=off like the rest of the library: expressions are evaluated as written.
#include <math.h>
#include <string.h>

#include "GraphMatRuntime.h"
#include "gm_internal.hpp"
#include "gm_run_fixed.hpp"

#define HD __host__ __device__
#define HDI __host__ __device__ __forceinline__

namespace gm {

extern int g_force_ordered;
// gm_set_option("lda_tile", 16 | 32 | 64): edges per step of k_lda_multiply (results do not depend on it).  Measured on 5e7 tokens
// (profiles/lda_k20.md): tile 16 / 32 / 64 -> 33.1 / 18.2 / 11.8 ms per iteration: phase A's 40 divisions per edge want every lane busy
int g_lda_tile = GM_LDA_TILE_DEFAULT;

constexpr int kLdaK = 20;
constexpr int kLdaStride = sizeof(gm_lda20_t) / 8;  // a vertex record in doubles
static_assert(sizeof(gm_lda20_t) == 176 && offsetof(gm_lda20_t, type) == 160 && offsetof(gm_lda20_t, token_loglik) == 168,
              "gm_lda20_t: the reference's LatentVector<20>");

// ---------------- the arithmetic of one edge ------------------------------------------------------------------------
// glibc's rand_r (stdlib/rand_r.c): three steps of a 32-bit linear congruential generator, 11 + 10 + 10 bits
HDI int lda_rand_r(unsigned int& seed) {
  unsigned int n = seed;
  n = n * 1103515245u + 12345u;
  unsigned int r = (n / 65536u) % 2048u;
  n = n * 1103515245u + 12345u;
  r = (r << 10) ^ ((n / 65536u) % 1024u);
  n = n * 1103515245u + 12345u;
  r = (r << 10) ^ ((n / 65536u) % 1024u);
  seed = n;
  return (int)r;
}
// init: K draws seeded with the edge value, normalised and scaled by it
HDI void lda_init_edge(int e, double* res) {
  unsigned int seed = (unsigned int)e;
  double sum = 0.0;
  for (int i = 0; i < kLdaK; i++) {
    const double g = (double)lda_rand_r(seed) / 2147483647;
    res[i] = g;
    sum += g;
  }
  for (int i = 0; i < kLdaK; i++) res[i] = res[i] / sum * (double)e;
}
// step: vN the destination's counts, mN the message (the source's counts), den[i] = global_N[i] + vocab * (eta - 1).
// res may be mN itself (mN[i] is read before res[i] is written).
HDI void lda_step_edge(const double* vN, const double* mN, double my, double other, const double* den, int e, double* res) {
  double sum = 0.0;
  for (int i = 0; i < kLdaK; i++) {
    const double g = (((vN[i] + my) - 1.0) * ((mN[i] + other) - 1.0)) / den[i];
    res[i] = g;
    sum += g;
  }
  for (int i = 0; i < kLdaK; i++) res[i] = res[i] / sum * (double)e;
}
HDI double lda_step_den(double global_n, double vocab, double eta) { return global_n + vocab * (eta - 1.0); }
// loglik: phi[i] of the destination, theta from the message
HDI double lda_phi(double vn, double global_n, int nterms, double eta) { return (vn + (eta - 1.0)) / (global_n + nterms * (eta - 1.0)); }
HDI double lda_loglik_edge(const double* phi, const double* mN, double eta, int e) {
  double sum = 0.0;
  for (int i = 0; i < kLdaK; i++) sum += mN[i] + (eta - 1.0);
  double dot = 0.0;
  for (int i = 0; i < kLdaK; i++) dot += phi[i] * ((mN[i] + (eta - 1.0)) / sum);
  return e * log(dot);
}

// ---------------- global_N: the sum of N over the word vertices -------------------------------------------------------
// A fixed two-level order that depends on the number of vertices only: level 1 cuts the rows into chunks of
// kLdaSumChunk, and inside a chunk row lane j of kLdaSumLanes adds rows j, j + 12, ... in order, then the 12 partial sums are
// added in order; level 2 is the same kernel, one workgroup, over the chunks' sums.  One implementation for both forms.
constexpr int kLdaSumLanes = 12;
constexpr int kLdaSumBlock = kLdaK * kLdaSumLanes;
constexpr int kLdaSumChunk = 768;

template <bool VERTICES /* items are vertex records and only words count; else plain rows of K sums */>
__global__ void __launch_bounds__(kLdaSumBlock)
k_lda_sum(const double* __restrict__ src, int64_t n, int64_t chunk, double* __restrict__ out) {
  __shared__ double s_p[kLdaSumLanes][kLdaK];
  const int k = threadIdx.x % kLdaK, j = threadIdx.x / kLdaK;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  double a = 0.0;
  for (int64_t r = lo + j; r < hi; r += kLdaSumLanes) {
    const double* p = src + r * (VERTICES ? kLdaStride : kLdaK);
    double t = p[k];
    if (VERTICES && *reinterpret_cast<const char*>(p + kLdaK) != 'w') t = 0.0;
    a += t;
  }
  s_p[j][k] = a;
  __syncthreads();
  if (j == 0) {
    double t = s_p[0][k];
    for (int q = 1; q < kLdaSumLanes; q++) t += s_p[q][k];
    out[(int64_t)blockIdx.x * kLdaK + k] = t;
  }
}
// enqueue both levels; *d_gn (device, K doubles, in workspace slot GM_WS_LDA_SUMS) holds the sums when the stream gets there
static int lda_global_n(gm_graph_t* g, const gm_lda20_t* d_vp, double** d_gn, hipStream_t s) {
  const int64_t n = g->desc.row_hi - g->desc.row_lo;
  const int64_t nchunks = (n + kLdaSumChunk - 1) / kLdaSumChunk;
  void* p = nullptr;
  int rc;
  if ((rc = gm_graph_workspace(g, GM_WS_LDA_SUMS, (size_t)(nchunks + 1) * kLdaK * 8 + 64, &p))) return rc;
  double* part = (double*)p;
  *d_gn = part + nchunks * kLdaK;
  hipLaunchKernelGGL((k_lda_sum<true>), dim3((unsigned)nchunks), dim3(kLdaSumBlock), 0, s, (const double*)d_vp, n, (int64_t)kLdaSumChunk, part);
  hipLaunchKernelGGL((k_lda_sum<false>), dim3(1), dim3(kLdaSumBlock), 0, s, (const double*)part, nchunks, nchunks, *d_gn);
  return GM_OK;
}
static int lda_global_n_to_host(gm_graph_t* g, const gm_lda20_t* d_vp, double* h_out, hipStream_t s) {
  double* d_gn = nullptr;
  int rc;
  if ((rc = lda_global_n(g, d_vp, &d_gn, s))) return rc;
  GM_TRY_HIP(hipMemcpyAsync(h_out, d_gn, kLdaK * 8, hipMemcpyDeviceToHost, s));
  GM_TRY_HIP(hipStreamSynchronize(s));
  return GM_OK;
}

// ---------------- the generic programs ------------------------------------------------------------------------------
struct LdaV : gm_lda20_t {
  HD bool operator!=(const LdaV& p) const {
    bool result = false;
    for (int i = 0; i < kLdaK; i++)
      if (p.N[i] != N[i]) result = true;
    return result || p.token_loglik != token_loglik;
  }
};

struct LdaInitP : GraphMat::GraphProgram<int, LdaV, LdaV, int> {
  LdaInitP() {
    this->order = GraphMat::ALL_EDGES;
    this->activity = GraphMat::ALL_VERTICES;
    this->process_message_requires_vertexprop = false;
  }
  HD void reduce_function(LdaV& a, const LdaV& b) const { for (int i = 0; i < kLdaK; i++) a.N[i] += b.N[i]; }
  HD void process_message(const int&, const int e, const LdaV&, LdaV& res) const {
    lda_init_edge(e, res.N);
    res.type = 0;
    res.token_loglik = 0.0;
  }
  HD bool send_message(const LdaV&, int& m) const { m = 0; return true; }
  HD void apply(const LdaV& y, LdaV& vp) { for (int i = 0; i < kLdaK; i++) vp.N[i] = y.N[i]; }
};

struct LdaP : GraphMat::GraphProgram<LdaV, LdaV, LdaV, int> {
  double alpha, eta, vocab;
  double global_N[kLdaK], den[kLdaK];
  // host side of the per-iteration hook (meaningless bytes on the device)
  gm_graph_t* g;
  const gm_lda20_t* d_vp;
  hipStream_t s;
  int rc;
  LdaP(double a, double e, double v, gm_graph_t* g_, const gm_lda20_t* vp_, hipStream_t s_) : alpha(a), eta(e), vocab(v), g(g_), d_vp(vp_), s(s_), rc(GM_OK) {
    this->order = GraphMat::ALL_EDGES;
    this->activity = GraphMat::ALL_VERTICES;
  }
  HD void reduce_function(LdaV& a, const LdaV& b) const { for (int i = 0; i < kLdaK; i++) a.N[i] += b.N[i]; }
  HD void process_message(const LdaV& m, const int e, const LdaV& vp, LdaV& res) const {
    const bool doc = vp.type == 'd';
    lda_step_edge(vp.N, m.N, doc ? alpha : eta, doc ? eta : alpha, den, e, res.N);
    res.type = 0;
    res.token_loglik = 0.0;
  }
  HD bool send_message(const LdaV& vp, LdaV& m) const { m = vp; return true; }
  HD void apply(const LdaV& y, LdaV& vp) { for (int i = 0; i < kLdaK; i++) vp.N[i] = y.N[i]; }
  // global_N of the state the next iteration starts from (the engine captures the program anew every iteration)
  void refresh() {
    if (rc == GM_OK) rc = lda_global_n_to_host(g, d_vp, global_N, s);
    for (int i = 0; i < kLdaK; i++) den[i] = lda_step_den(global_N[i], vocab, eta);
  }
  void do_every_iteration(int) { refresh(); }
};

struct LdaLLP : GraphMat::GraphProgram<LdaV, double, LdaV, int> {
  double eta;
  int nterms;
  double global_N[kLdaK];
  LdaLLP(double e, int nt) : eta(e), nterms(nt) {
    this->order = GraphMat::OUT_EDGES;
    this->activity = GraphMat::ALL_VERTICES;
  }
  HD void reduce_function(double& a, const double& b) const { a += b; }
  HD void process_message(const LdaV& m, const int e, const LdaV& vp, double& res) const {
    double phi[kLdaK];
    for (int i = 0; i < kLdaK; i++) phi[i] = lda_phi(vp.N[i], global_N[i], nterms, eta);
    res = lda_loglik_edge(phi, m.N, eta, e);
  }
  HD bool send_message(const LdaV& vp, LdaV& m) const { m = vp; return true; }
  HD void apply(const double& y, LdaV& vp) { vp.token_loglik = y; }
};

// ---------------- the dedicated kernels -------------------------------------------------------------------------------
constexpr int kLdaBlock = 256;
__global__ void __launch_bounds__(kLdaBlock)
k_lda_send(const double* __restrict__ vp, double* __restrict__ x, int n) {  // x[v][0..K) = vp[v].N
  const int64_t i = (int64_t)blockIdx.x * kLdaBlock + threadIdx.x;
  if (i >= (int64_t)n * kLdaK) return;
  const int v = (int)(i / kLdaK), c = (int)(i % kLdaK);
  x[i] = vp[(int64_t)v * kLdaStride + c];
}
__global__ void __launch_bounds__(kLdaBlock)
k_lda_apply(const double* __restrict__ y, const uint32_t* __restrict__ bits, double* __restrict__ vp, int n) {  // N = y where a message arrived
  const int64_t i = (int64_t)blockIdx.x * kLdaBlock + threadIdx.x;
  if (i >= (int64_t)n * kLdaK) return;
  const int v = (int)(i / kLdaK), c = (int)(i % kLdaK);
  if ((bits[v >> 5] >> (v & 31)) & 1u) vp[(int64_t)v * kLdaStride + c] = y[i];
}
__global__ void __launch_bounds__(kLdaBlock)
k_lda_loglik_apply(const double* __restrict__ y1, const uint32_t* __restrict__ bits, double* __restrict__ vp, int n) {
  const int v = blockIdx.x * kLdaBlock + threadIdx.x;
  if (v < n && ((bits[v >> 5] >> (v & 31)) & 1u)) vp[(int64_t)v * kLdaStride + kLdaStride - 1] = y1[v];  // token_loglik
}

__device__ __forceinline__ double lda_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}
// the wave's LDS accesses before and after stay on their sides (LDS is in order per wave)
__device__ __forceinline__ void lda_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// MODE 0: step, products summed into y (row stride K);  MODE 1: loglik, count * log(phi . theta) summed into y[row];
// MODE 2: init (nothing is gathered: the products depend on the edge values only), summed into y like MODE 0.
// One wave per row, TILE edges per step.  The step's message rows (160 bytes each) are fetched once, 16 bytes a lane, and
// parked in the wave's LDS tile; the next step's column ids, values and rows are in flight while this step computes:
//   phase A  lane = edge: its message row (LDS) against the row's own vector (LDS, broadcast), 40 divisions, the products
//            written over the message row;
//   phase B  lane = component: the tile's edges in stored order, y += product.
// a and b: alpha and eta of the step; eta and nterms of loglik.
constexpr int kLdaMulBlock = 128;
template <int MODE, int TILE>
__global__ void __launch_bounds__(kLdaMulBlock)
k_lda_multiply(gm_csr_t A, const double* __restrict__ x, const double* __restrict__ vp, double* __restrict__ y,
               const uint32_t* __restrict__ prev_bits, int accumulate, const double* __restrict__ gn, double a, double b, double scale) {
  static_assert(TILE >= 1 && TILE <= 64, "a lane per edge of the tile");
  constexpr int K = kLdaK;
  constexpr int XS = K + 1;       // LDS row stride in doubles (odd: the lanes of phase A, a row each, spread over the banks)
  constexpr int PARTS = K / 2;    // 16-byte pieces of a message row
  constexpr int NLD = (TILE * PARTS + 63) / 64;  // load instructions per tile
  constexpr int WPB = kLdaMulBlock / 64;
  __shared__ double s_v[WPB][K], s_d[WPB][K];
  __shared__ double s_x[WPB][TILE][XS];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * WPB + wv;
  if (row >= A.nrows) return;
  const int64_t e0 = A.rowptr[row], e1 = A.rowptr[row + 1];
  if (e1 == e0) return;
  const double* vrow = vp + (int64_t)row * kLdaStride;
  double my = 0.0, other = 0.0;
  if (MODE == 0) {
    const bool doc = *reinterpret_cast<const char*>(vrow + K) == 'd';
    my = doc ? a : b;
    other = doc ? b : a;
    if (lane < K) {
      s_v[wv][lane] = vrow[lane];
      s_d[wv][lane] = lda_step_den(gn[lane], scale, b);
    }
  } else if (MODE == 1) {
    if (lane < K) s_v[wv][lane] = lda_phi(vrow[lane], gn[lane], (int)scale, a);
  }
  bool has = accumulate && ((prev_bits[row >> 5] >> (row & 31)) & 1u);
  double acc = 0.0;
  if (has) {
    if (MODE == 1) acc = y[row];
    else if (lane < K) acc = y[(int64_t)row * K + lane];
  }
  const int* vals = (const int*)A.vals;

  int col = 0, val = 0;
  double2 q[NLD];
  auto fetch = [&](int64_t base) {  // column ids + values of the tile, then its message rows
    const int n = (int)((e1 - base) < TILE ? (e1 - base) : TILE);
    col = 0;
    val = 0;
    if (lane < n) {
      if (MODE != 2) col = __builtin_nontemporal_load(A.colidx + base + lane);
      val = __builtin_nontemporal_load(vals + base + lane);
    }
    if (MODE != 2) {
#pragma unroll
      for (int r = 0; r < NLD; r++) {
        const int idx = r * 64 + lane, e = idx / PARTS, part = idx % PARTS;
        const int c = __shfl(col, e);
        q[r] = make_double2(0.0, 0.0);
        if (e < n) q[r] = *reinterpret_cast<const double2*>(x + (int64_t)c * K + 2 * part);
      }
    }
  };
  fetch(e0);
  for (int64_t base = e0; base < e1; base += TILE) {
    const int n = (int)((e1 - base) < TILE ? (e1 - base) : TILE);
    const int my_val = val;
    lda_wave_sync();  // phase B of the previous tile has read it
    if (MODE != 2) {
#pragma unroll
      for (int r = 0; r < NLD; r++) {
        const int idx = r * 64 + lane, e = idx / PARTS, part = idx % PARTS;
        if (e < TILE) {
          s_x[wv][e][2 * part] = q[r].x;
          s_x[wv][e][2 * part + 1] = q[r].y;
        }
      }
    }
    lda_wave_sync();
    if (base + TILE < e1) fetch(base + TILE);  // the next tile flies during the phases below
    // phase A
    double ll = 0.0;
    if (lane < n) {
      double* xr = s_x[wv][lane];
      if (MODE == 0) lda_step_edge(s_v[wv], xr, my, other, s_d[wv], my_val, xr);
      else if (MODE == 1) ll = lda_loglik_edge(s_v[wv], xr, a, my_val);
      else lda_init_edge(my_val, xr);
    }
    if (MODE == 1) {
      for (int e = 0; e < n; e++) {
        const double t = lda_readlane(ll, e);
        acc = has ? acc + t : t;
        has = true;
      }
    } else {
      lda_wave_sync();
      // phase B
      if (lane < K) {
        bool h = has;
        for (int e = 0; e < n; e++) {
          const double r = s_x[wv][e][lane];
          acc = h ? acc + r : r;
          h = true;
        }
      }
      has = true;
    }
  }
  if (MODE == 1) {
    if (lane == 0) y[row] = acc;
  } else if (lane < K) {
    y[(int64_t)row * K + lane] = acc;
  }
}

template <int MODE>
static void lda_launch_multiply(hipStream_t s, int n, const gm_csr_t& A, const double* x, const double* vp, double* y, const uint32_t* prev_bits,
                                int accumulate, const double* gn, double a, double b, double scale) {
  const dim3 grid((n + kLdaMulBlock / 64 - 1) / (kLdaMulBlock / 64)), block(kLdaMulBlock);
  if (g_lda_tile == 16) hipLaunchKernelGGL((k_lda_multiply<MODE, 16>), grid, block, 0, s, A, x, vp, y, prev_bits, accumulate, gn, a, b, scale);
  else if (g_lda_tile == 32) hipLaunchKernelGGL((k_lda_multiply<MODE, 32>), grid, block, 0, s, A, x, vp, y, prev_bits, accumulate, gn, a, b, scale);
  else hipLaunchKernelGGL((k_lda_multiply<MODE, 64>), grid, block, 0, s, A, x, vp, y, prev_bits, accumulate, gn, a, b, scale);
}

struct LdaScratch {
  double *x, *y;
  int n, egrid;
};
static int lda_scratch(gm_graph_t* g, LdaScratch* w) {
  const gm_graph_desc_t& d = g->desc;
  w->n = d.row_hi - d.row_lo;
  void *px = nullptr, *py = nullptr;
  int rc;
  if ((rc = gm_graph_workspace(g, GM_WS_X, (size_t)d.ndevice * kLdaK * 8 + 64, &px))) return rc;
  if ((rc = gm_graph_workspace(g, GM_WS_Y, (size_t)w->n * kLdaK * 8 + 64, &py))) return rc;
  w->x = (double*)px;
  w->y = (double*)py;
  w->egrid = (int)(((int64_t)w->n * kLdaK + kLdaBlock - 1) / kLdaBlock);
  return GM_OK;
}

static int run_lda_init_wide(gm_graph_t* g, gm_lda20_t* d_vp, hipStream_t s) {
  LdaScratch w;
  int rc;
  if ((rc = lda_scratch(g, &w))) return rc;
  double* vp = (double*)d_vp;
  lda_launch_multiply<2>(s, w.n, g->out.view, w.x, vp, w.y, nullptr, 0, nullptr, 0.0, 0.0, 0.0);
  lda_launch_multiply<2>(s, w.n, g->in.view, w.x, vp, w.y, g->out.rowbits, 1, nullptr, 0.0, 0.0, 0.0);
  hipLaunchKernelGGL(k_lda_apply, dim3(w.egrid), dim3(kLdaBlock), 0, s, (const double*)w.y, (const uint32_t*)g->rowbits_all, vp, w.n);
  GM_TRY_HIP(hipStreamSynchronize(s));
  return GM_OK;
}

// fixed iteration count; global_N stays on the device between the iterations
static int run_lda_wide(gm_graph_t* g, gm_lda20_t* d_vp, double alpha, double eta, double vocab, int iterations, double* h_gn, hipStream_t s) {
  LdaScratch w;
  int rc;
  if ((rc = lda_scratch(g, &w))) return rc;
  double* vp = (double*)d_vp;
  double* d_gn = nullptr;
  gm_run_stats_t st;
  memset(&st, 0, sizeof(st));
  hipEvent_t ev0, ev1;
  GM_TRY_HIP(hipEventCreate(&ev0));
  GM_TRY_HIP(hipEventCreate(&ev1));
  GM_TRY_HIP(hipEventRecord(ev0, s));
  if ((rc = lda_global_n(g, d_vp, &d_gn, s))) return rc;
  for (int it = 0; it < iterations; it++) {
    hipLaunchKernelGGL(k_lda_send, dim3(w.egrid), dim3(kLdaBlock), 0, s, (const double*)vp, w.x, w.n);
    lda_launch_multiply<0>(s, w.n, g->out.view, w.x, vp, w.y, nullptr, 0, d_gn, alpha, eta, vocab);
    lda_launch_multiply<0>(s, w.n, g->in.view, w.x, vp, w.y, g->out.rowbits, 1, d_gn, alpha, eta, vocab);
    hipLaunchKernelGGL(k_lda_apply, dim3(w.egrid), dim3(kLdaBlock), 0, s, (const double*)w.y, (const uint32_t*)g->rowbits_all, vp, w.n);
    if ((rc = lda_global_n(g, d_vp, &d_gn, s))) return rc;
  }
  GM_TRY_HIP(hipEventRecord(ev1, s));
  if (h_gn) GM_TRY_HIP(hipMemcpyAsync(h_gn, d_gn, kLdaK * 8, hipMemcpyDeviceToHost, s));
  GM_TRY_HIP(hipStreamSynchronize(s));
  GM_TRY_HIP(hipEventElapsedTime(&st.total_ms, ev0, ev1));
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  st.iterations = iterations;
  g->stats = st;
  return GM_OK;
}

static int run_lda_loglik_wide(gm_graph_t* g, gm_lda20_t* d_vp, double eta, int nterms, hipStream_t s) {
  LdaScratch w;
  int rc;
  if ((rc = lda_scratch(g, &w))) return rc;
  double* vp = (double*)d_vp;
  double* d_gn = nullptr;
  if ((rc = lda_global_n(g, d_vp, &d_gn, s))) return rc;
  hipLaunchKernelGGL(k_lda_send, dim3(w.egrid), dim3(kLdaBlock), 0, s, (const double*)vp, w.x, w.n);
  lda_launch_multiply<1>(s, w.n, g->out.view, w.x, vp, w.y, nullptr, 0, d_gn, eta, 0.0, (double)nterms);
  hipLaunchKernelGGL(k_lda_loglik_apply, dim3((w.n + kLdaBlock - 1) / kLdaBlock), dim3(kLdaBlock), 0, s, (const double*)w.y,
                     (const uint32_t*)g->out.rowbits, vp, w.n);
  GM_TRY_HIP(hipStreamSynchronize(s));
  return GM_OK;
}

// argument errors first (nothing on the GPU is touched), then what the LDA entry points need of the graph
static int lda_check(const char* fn, const gm_graph_t* g, const void* d_vp, int K) {
  if (!g || !d_vp) { set_error("%s: null graph or vertex state", fn); return GM_ERR_INVALID; }
  if (K != kLdaK) { set_error("%s: K=%d is not in the fixed menu (K=20, fp64)", fn, K); return GM_ERR_UNSUPPORTED; }
  const gm_graph_desc_t& d = g->desc;
  if (d.row_lo != 0 || d.row_hi != d.ndevice || g->xfn != nullptr) { set_error("%s: sharded graphs are not supported", fn); return GM_ERR_UNSUPPORTED; }
  if (!g->out.present || !g->in.present || !g->rowbits_all) { set_error("%s: needs a graph built with both directions", fn); return GM_ERR_UNSUPPORTED; }
  if (d.val_bytes != 4 || !g->out.vals || !g->in.vals) { set_error("%s: needs 4-byte edge values (the token counts)", fn); return GM_ERR_UNSUPPORTED; }
  return GM_OK;
}

}  // namespace gm

extern "C" {

int gm_lda_edge_init(int edge_value, int K, double* h_out) {
  if (!h_out) { gm::set_error("gm_lda_edge_init: null argument"); return GM_ERR_INVALID; }
  if (K != gm::kLdaK) { gm::set_error("gm_lda_edge_init: K=%d is not in the fixed menu (K=20, fp64)", K); return GM_ERR_UNSUPPORTED; }
  gm::lda_init_edge(edge_value, h_out);
  return GM_OK;
}

int gm_run_lda_init(gm_graph_t* g, gm_lda20_t* d_vp, int K, gm_stream_t stream) {
  int rc;
  if ((rc = gm::lda_check("gm_run_lda_init", g, d_vp, K))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (!gm::g_force_ordered) return gm::run_lda_init_wide(g, d_vp, s);
  gm::LdaInitP p;
  return gm::run_fixed(p, g, (gm::LdaV*)d_vp, (uint32_t*)nullptr, 1, nullptr, s);
}

int gm_lda_global_n(gm_graph_t* g, const gm_lda20_t* d_vp, int K, double* h_out, gm_stream_t stream) {
  int rc;
  if ((rc = gm::lda_check("gm_lda_global_n", g, d_vp, K))) return rc;
  if (!h_out) { gm::set_error("gm_lda_global_n: null argument"); return GM_ERR_INVALID; }
  return gm::lda_global_n_to_host(g, d_vp, h_out, (hipStream_t)stream);
}

int gm_run_lda(gm_graph_t* g, gm_lda20_t* d_vp, int K, double alpha, double eta, double vocab_size, int iterations, int* iters_done,
               double* h_global_N, gm_stream_t stream) {
  if (g && d_vp && iterations < 1) { gm::set_error("gm_run_lda: iterations must be at least 1 (a fixed count)"); return GM_ERR_INVALID; }
  int rc;
  if ((rc = gm::lda_check("gm_run_lda", g, d_vp, K))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (!gm::g_force_ordered) {
    if ((rc = gm::run_lda_wide(g, d_vp, alpha, eta, vocab_size, iterations, h_global_N, s))) return rc;
    if (iters_done) *iters_done = iterations;
    return GM_OK;
  }
  gm::LdaP p(alpha, eta, vocab_size, g, d_vp, s);
  p.refresh();  // the sums of the state the first iteration starts from
  if (p.rc) return p.rc;
  if ((rc = gm::run_fixed(p, g, (gm::LdaV*)d_vp, (uint32_t*)nullptr, iterations, iters_done, s))) return rc;
  if (p.rc) return p.rc;
  if (h_global_N) memcpy(h_global_N, p.global_N, sizeof(p.global_N));
  return GM_OK;
}

int gm_run_lda_loglik(gm_graph_t* g, gm_lda20_t* d_vp, int K, double eta, int nterms, double* h_total, gm_stream_t stream) {
  int rc;
  if ((rc = gm::lda_check("gm_run_lda_loglik", g, d_vp, K))) return rc;
  if (!h_total) { gm::set_error("gm_run_lda_loglik: null argument"); return GM_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  if (!gm::g_force_ordered) {
    if ((rc = gm::run_lda_loglik_wide(g, d_vp, eta, nterms, s))) return rc;
  } else {
    gm::LdaLLP p(eta, nterms);
    if ((rc = gm::lda_global_n_to_host(g, d_vp, p.global_N, s))) return rc;
    if ((rc = gm::run_fixed(p, g, (gm::LdaV*)d_vp, (uint32_t*)nullptr, 1, nullptr, s))) return rc;
  }
  return gm_reduce_sum_f64((const double*)d_vp + gm::kLdaStride - 1, g->desc.row_hi - g->desc.row_lo, gm::kLdaStride, h_total, stream);
}

}  // extern "C"
