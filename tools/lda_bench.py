#!/usr/bin/env python3
"""LDA timing (K = 20 fp64): the dedicated kernels against the generic engine (option force_ordered).

Synthetic corpus: documents 1..D, words D+1..D+T, `tokens` edges document -> word with counts 1..5.  Documents are drawn
uniformly; a word's popularity is Zipf-like, proportional to 1 / (rank + shift), so that word rows of 10^5 edges and more
exist next to rows of a handful (shift = 0 is the plain Zipf law, whose most frequent word alone owns ~8% of the tokens; a
row is folded in order by one wave, so a corpus with its stop words left in is bound by that single row).
One iteration = send + ALL_EDGES multiply (both directions) + apply + the global sums.  Reports ms per iteration, edge
visits per second and gathered bytes per second (160 bytes per edge visit), and checks that the dedicated form's final
state equals the generic form's bit for bit."""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1 << 20)
    ap.add_argument("--terms", type=int, default=1 << 16)
    ap.add_argument("--tokens", type=int, default=50_000_000)
    ap.add_argument("--shift", type=float, default=50.0, help="word popularity ~ 1 / (rank + shift)")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--tiles", default="16,32,64", help="values of option lda_tile to time the dedicated form with")
    ap.add_argument("--skip-generic", action="store_true", help="dedicated form only (no comparison)")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    from graphmat_amd import api, _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    D, T, E = args.docs, args.terms, args.tokens
    nv = D + T
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    src = torch.randint(1, D + 1, (E,), generator=gen, device=dev).to(torch.int32)
    cdf = torch.cumsum(1.0 / (torch.arange(T, dtype=torch.float64, device=dev) + 1.0 + args.shift), 0)
    cdf /= cdf[-1].clone()
    word = torch.searchsorted(cdf, torch.rand(E, generator=gen, device=dev, dtype=torch.float64)).clamp_(max=T - 1)
    dst = (D + 1 + word).to(torch.int32)
    val = torch.randint(1, 6, (E,), generator=gen, device=dev).to(torch.int32)
    longest = int(torch.bincount(word, minlength=T).max())
    del word, cdf
    g = api.Graph(nv, src, dst, val)
    del src, dst, val
    alpha, eta = 1.0, 5.0
    it = C.c_int(0)

    st0 = g._lda_to_device(np.zeros((nv, 20)), D)
    _lib.check(L.gm_run_lda_init(g.h, st0.data_ptr(), 20, None))
    res = {"docs": D, "terms": T, "tokens": E, "shift": args.shift, "longest_word_row": longest, "iters": args.iters, "forms": []}
    print("LDA K=20 fp64: docs=%d terms=%d tokens=%d, longest word row %d edges" % (D, T, E, longest), flush=True)

    def run(label):
        st = st0.clone()
        warm = st0.clone()
        _lib.check(L.gm_run_lda(g.h, warm.data_ptr(), 20, alpha, eta, float(T), 1, C.byref(it), None, None))
        del warm
        torch.cuda.synchronize(); t0 = time.perf_counter()
        _lib.check(L.gm_run_lda(g.h, st.data_ptr(), 20, alpha, eta, float(T), args.iters, C.byref(it), None, None))
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / args.iters
        visits, gathered = 2 * E, 2 * E * 160
        print("  %-22s %9.2f ms/iteration, %6.2f G edge-visits/s, gathered %.1f GB -> %6.0f GB/s"
              % (label, dt * 1e3, visits / dt / 1e9, gathered / 1e9, gathered / dt / 1e9), flush=True)
        res["forms"].append({"form": label, "ms_per_iteration": dt * 1e3, "edge_visits_per_s": visits / dt, "gathered_bytes_per_s": gathered / dt})
        return st

    final = None
    for tile in [int(x) for x in args.tiles.split(",") if x]:
        _lib.check(L.gm_set_option(b"lda_tile", tile))
        st = run("dedicated, tile %d" % tile)
        if final is not None:
            assert torch.equal(st.view(torch.int64), final.view(torch.int64)), "the tile size changed the result"
        final = st
    L.gm_reset_options()
    if not args.skip_generic:
        _lib.check(L.gm_set_option(b"force_ordered", 1))
        st = run("generic engine")
        L.gm_reset_options()
        same = torch.equal(st.view(torch.int64), final.view(torch.int64))
        res["dedicated_equals_generic"] = bool(same)
        print("  final state of the dedicated form %s the generic form's" % ("equals, bit for bit," if same else "DIFFERS from"), flush=True)
        assert same
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
