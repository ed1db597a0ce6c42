// gm_run_fixed.hpp -- how the fixed-menu translation units (gm_programs.hip, gm_lda.hip) hand a program to the common engine
#pragma once
#include "GraphMatRuntime.h"
#include "gm_internal.hpp"

namespace gm {

// run a program on caller-provided device state through the common engine
template <class P, class V>
int run_fixed(P& prog, gm_graph_t* g, V* d_vp, uint32_t* d_active, int iterations, int* iters_done, hipStream_t s) {
  typedef typename GraphMat::detail::types_of<P>::type PT;
  typedef typename PT::msg T;
  typedef typename PT::red U;
  if (!g || !d_vp) { set_error("gm_run_*: null graph or vertex state"); return GM_ERR_INVALID; }
  const gm_graph_desc_t& d = g->desc;
  const int rows = d.row_hi - d.row_lo;
  const auto order = prog.getOrder();
  if ((order != GraphMat::IN_EDGES && !g->out.present) || (order != GraphMat::OUT_EDGES && !g->in.present)) {
    set_error("gm_run_*: graph was built without the adjacency direction this program needs");
    return GM_ERR_INVALID;
  }
  void *p0, *p1, *p2, *p3, *p5;
  int rc;
  if ((rc = gm_graph_workspace(g, GM_WS_X, (size_t)d.ndevice * sizeof(T) + 16, &p0))) return rc;
  if ((rc = gm_graph_workspace(g, GM_WS_XBITS, ((size_t)(d.ndevice + 31) / 32 + 2) * 4, &p1))) return rc;
  if ((rc = gm_graph_workspace(g, GM_WS_Y, (size_t)rows * sizeof(U) + 16, &p2))) return rc;
  if ((rc = gm_graph_workspace(g, GM_WS_YBITS, ((size_t)(rows + 31) / 32 + 2) * 4, &p3))) return rc;
  if (!d_active) {
    const size_t nw = (size_t)(rows + 31) / 32;
    if ((rc = gm_graph_workspace(g, GM_WS_ALL_ACTIVE, (nw + 2) * 4, &p5))) return rc;
    d_active = (uint32_t*)p5;
    hipLaunchKernelGGL(GraphMat::dev::k_fill_u32, dim3(GraphMat::detail::grid_for((int64_t)nw)),
                       dim3(GraphMat::dev::kBlock), 0, s, d_active, (int64_t)nw, 0xffffffffu);
    if (rows & 31) {
      uint32_t tail = (1u << (rows & 31)) - 1u;
      GM_TRY_HIP(hipMemcpyAsync(d_active + nw - 1, &tail, 4, hipMemcpyHostToDevice, s));
      GM_TRY_HIP(hipStreamSynchronize(s));
    }
  }
  int it = GraphMat::detail::run_on_device<P, T, U, V, int>(&prog, g, order, prog.getActivity(),
                                                             prog.getProcessMessageRequiresVertexprop(), d_vp, d_active,
                                                             (T*)p0, (uint32_t*)p1, (U*)p2, (uint32_t*)p3, iterations, s);
  if (iters_done) *iters_done = it;
  return GM_OK;
}

}  // namespace gm
