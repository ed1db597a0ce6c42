"""LDA (K = 20, fp64) on the GPU against a numpy restatement of its semantics, written in this file.

The restatement is this file's own (no oracle program exists for LDA): it follows the description of the three vertex
programs (init, step, log-likelihood; IEEE fp64) and is vectorised across edges, with explicit Python loops over the 20
components wherever the order of a sum matters (never np.sum for an ordered sum).  A row's fold is np.add.at over its
edges in stored order -- ufunc.at applies in index order -- first the OUT-direction adjacency's, then the
IN-direction's; the stored order comes from Graph.csr_to_host, which other tests pin against the oracle.  Starting the
fold from 0.0 instead of assigning the first product gives the same bits because no product is -0.0.
An adjacency is the triple (rows, cols, vals) of its edges in stored order, rows and cols in device order.

Every check runs for the dedicated kernels (the default) and for the generic programs (option force_ordered = 1).
"""
import ctypes as C
import math

import numpy as np
import pytest

K = 20
_libc = None


def rand_r(seed):
    """glibc's rand_r on a ctypes c_uint seed (updated in place)."""
    global _libc
    if _libc is None:
        _libc = C.CDLL("libc.so.6")
        _libc.rand_r.argtypes = [C.POINTER(C.c_uint)]
        _libc.rand_r.restype = C.c_int
    return _libc.rand_r(C.byref(seed))


def init_product(e):
    """The init product of one edge of value e: [20] float64."""
    seed = C.c_uint(int(e) & 0xFFFFFFFF)
    g = []
    s = np.float64(0.0)
    for i in range(K):
        gi = np.float64(rand_r(seed)) / np.float64(2147483647)
        g.append(gi)
        s = s + gi
    return np.array([gi / s * np.float64(e) for gi in g], np.float64)


def edges_of(rp, ci, vv):
    """(rows, cols, vals) of a CSR in stored order."""
    rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    return rows, ci.astype(np.int64), vv.astype(np.int64)


def _fold(nrows, passes):
    """passes: [(rows, products[ne, 20])] in fold order -> (y[nrows, 20], received[nrows])"""
    y = np.zeros((nrows, K), np.float64)
    got = np.zeros(nrows, bool)
    for rows, prod in passes:
        np.add.at(y, rows, prod)
        got[rows] = True
    return y, got


def init(nrows, adj_out, adj_in):
    """N after the init pass from an all-zero state: [nrows, 20]."""
    passes = []
    for rows, _, vals in (adj_out, adj_in):
        uniq, inv = np.unique(vals, return_inverse=True)
        table = np.array([init_product(e) for e in uniq], np.float64).reshape(len(uniq), K)
        passes.append((rows, table[inv]))
    y, got = _fold(nrows, passes)
    return np.where(got[:, None], y, 0.0)


def step(N, is_doc, gN, adj_out, adj_in, alpha, eta, vocab):
    """One LDA iteration on N [nrows, 20] (device order) with the given global sums."""
    den = [np.float64(gN[i]) + np.float64(vocab) * (np.float64(eta) - 1.0) for i in range(K)]
    passes = []
    for rows, cols, vals in (adj_out, adj_in):
        v, m = N[rows], N[cols]
        my = np.where(is_doc[rows], np.float64(alpha), np.float64(eta))
        other = np.where(is_doc[rows], np.float64(eta), np.float64(alpha))
        g = np.empty((len(rows), K), np.float64)
        s = np.zeros(len(rows), np.float64)
        for i in range(K):
            g[:, i] = (((v[:, i] + my) - 1.0) * ((m[:, i] + other) - 1.0)) / den[i]
            s = s + g[:, i]
        e = vals.astype(np.float64)
        prod = np.empty_like(g)
        for i in range(K):
            prod[:, i] = g[:, i] / s * e
        passes.append((rows, prod))
    y, got = _fold(len(N), passes)
    return np.where(got[:, None], y, N)


def global_n(N, is_word):
    """Sum of N over the word rows, component by component, in row order (the library may use any order)."""
    out = np.zeros(K, np.float64)
    for r in np.nonzero(is_word)[0]:
        out = out + N[r]
    return out


def loglik(N, gN, adj_out, eta, nterms):
    """token_loglik [nrows] after the log-likelihood pass (rows that receive nothing: 0)."""
    rows, cols, vals = adj_out
    v, m = N[rows], N[cols]
    e1 = np.float64(eta) - 1.0
    theta = np.empty((len(rows), K), np.float64)
    s = np.zeros(len(rows), np.float64)
    for i in range(K):
        theta[:, i] = m[:, i] + e1
        s = s + theta[:, i]
    dot = np.zeros(len(rows), np.float64)
    for i in range(K):
        nk = np.float64(gN[i]) + nterms * e1
        phi = (v[:, i] + e1) / nk
        dot = dot + phi * (theta[:, i] / s)
    res = vals.astype(np.float64) * np.log(dot)
    y = np.zeros(len(N), np.float64)
    np.add.at(y, rows, res)
    return y


# ---------------- corpora ---------------------------------------------------------------------------------------
pytestmark = pytest.mark.gpu
ALPHA, ETA = 1.0, 5.0
FORMS = (0, 1)  # force_ordered


def corpus_a():
    rng = np.random.default_rng(20)
    ndoc, nterms, ntok = 300, 60, 4000
    s = rng.integers(1, ndoc, ntok).astype(np.int32)             # documents 1..299: the last one is isolated
    d = (ndoc + rng.integers(1, nterms, ntok)).astype(np.int32)  # words 1..59: the last one is isolated
    v = rng.integers(1, 6, ntok).astype(np.int32)
    return ndoc, nterms, s, d, v


def corpus_b():
    ndoc, lens = 129, (1, 15, 16, 17, 63, 64, 65, 129)  # every tile boundary at 16 and 64, on both sides
    s = np.concatenate([np.arange(1, n + 1) for n in lens]).astype(np.int32)
    d = np.concatenate([np.full(n, ndoc + j + 1) for j, n in enumerate(lens)]).astype(np.int32)
    v = (np.arange(len(s)) % 5 + 1).astype(np.int32)
    return ndoc, len(lens), s, d, v


def corpus_c():
    rng = np.random.default_rng(11)
    ndoc, nterms, ntok = 9000, 2, 14000  # two giant word rows
    s = rng.integers(1, ndoc + 1, ntok).astype(np.int32)
    d = (ndoc + rng.integers(1, nterms + 1, ntok)).astype(np.int32)
    v = rng.integers(1, 6, ntok).astype(np.int32)
    return ndoc, nterms, s, d, v


class Case:
    """A corpus on the GPU plus what the restatement needs of it; reference results are computed once and kept."""

    def __init__(self, api, name, corpus, ref_threads=1):
        self.api, self.name = api, name
        self.ndoc, self.nterms, s, d, v = corpus
        self.nv = self.ndoc + self.nterms
        self.g = api.Graph(self.nv, s, d, v, ref_threads=ref_threads)
        self.adj_out = edges_of(*self.g.csr_to_host(api.GM_DIR_OUT))
        self.adj_in = edges_of(*self.g.csr_to_host(api.GM_DIR_IN))
        self.dov = self.g.dev_of_vertex.cpu().numpy()
        self.nrows = self.g.ndevice
        self.is_doc = np.zeros(self.nrows, bool)
        self.is_doc[self.dov[: self.ndoc]] = True
        deg = np.bincount(np.concatenate([s, d]), minlength=self.nv + 1)[1:]
        self.isolated = deg == 0
        self._memo = {}

    def to_dev(self, N):
        out = np.zeros((self.nrows, K), np.float64)
        out[self.dov] = N
        return out

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
            if isinstance(self._memo[key], np.ndarray):
                self._memo[key].setflags(write=False)
        return self._memo[key]

    def ref_init(self):
        return self.memo("init", lambda: init(self.nrows, self.adj_out, self.adj_in)[self.dov])

    def set_form(self, force_ordered):
        self.api._lib.lib().gm_set_option(b"force_ordered", force_ordered)


@pytest.fixture(scope="module")
def cases():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graphmat_amd import build
    build.build()
    from graphmat_amd import api
    return {"A1": Case(api, "A1", corpus_a(), 1), "A2": Case(api, "A2", corpus_a(), 2), "B": Case(api, "B", corpus_b()),
            "C": Case(api, "C", corpus_c())}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


# ---------------- the checks ------------------------------------------------------------------------------------
def test_giant_rows_present(cases):
    c = cases["C"]
    assert c.g.csr(c.api.GM_DIR_OUT).ngiant >= 2


@pytest.mark.parametrize("force", FORMS)
@pytest.mark.parametrize("name", ["A1", "B", "C"])
def test_init(cases, name, force):
    c = cases[name]
    c.set_form(force)
    N = c.g.lda_init(c.ndoc)
    assert same_bits(N, c.ref_init())
    assert np.isfinite(N).all() and (N[~c.isolated] > 0).all() and (N[c.isolated] == 0).all()
    if name == "A1":
        assert c.isolated[c.ndoc - 1] and c.isolated[c.nv - 1]


@pytest.mark.parametrize("name", ["A1", "B", "C"])
def test_global_sums(cases, name):
    c = cases[name]
    N0 = c.ref_init()
    gn = c.g.lda_global_n(N0, c.ndoc)
    again = c.g.lda_global_n(N0, c.ndoc)
    assert same_bits(gn, again)
    for k in range(K):
        exact = math.fsum(N0[c.ndoc:, k])
        rel = abs(gn[k] - exact) / exact
        print("%s global_N[%d]: relative deviation from fsum %.3g" % (name, k, rel))
        assert rel <= c.nv * 2.0 ** -53  # any order of a sum of non-negative terms stays inside this


@pytest.mark.parametrize("force", FORMS)
@pytest.mark.parametrize("name", ["A1", "A2", "B", "C"])
def test_one_step_exact(cases, name, force):
    c = cases[name]
    N0 = c.ref_init()
    gn = c.g.lda_global_n(N0, c.ndoc)
    ref = c.memo("step1", lambda: step(c.to_dev(N0), c.is_doc, gn, c.adj_out, c.adj_in, ALPHA, ETA, float(c.nterms))[c.dov])
    c.set_form(force)
    N1, gn1, it = c.g.lda(N0, c.ndoc, c.nterms, ALPHA, ETA, 1)
    assert it == 1
    diff = bits(N1) != bits(ref)
    assert not diff.any(), "%d of %d values differ, first at %s" % (diff.sum(), diff.size, np.argwhere(diff)[0])
    assert same_bits(N1[c.isolated], N0[c.isolated])


def three_iterations(c, force):
    def run():
        c.set_form(force)
        N3, gn3, it = c.g.lda(c.ref_init(), c.ndoc, c.nterms, ALPHA, ETA, 3)
        assert it == 3
        gn3.setflags(write=False)
        return N3, gn3
    return c.memo(("three", force), run)


@pytest.mark.parametrize("force", FORMS)
@pytest.mark.parametrize("name", ["A1", "B", "C"])
def test_iteration_structure(cases, name, force):
    """global_N is recomputed after every iteration's apply: one call of 3 iterations = 3 calls of 1, and the sums returned
    are those of the state returned."""
    c = cases[name]
    N3, gn3 = three_iterations(c, force)
    c.set_form(force)
    N = c.ref_init()
    for _ in range(3):
        N, gn, it = c.g.lda(N, c.ndoc, c.nterms, ALPHA, ETA, 1)
    assert same_bits(N, N3) and same_bits(gn, gn3)
    assert same_bits(c.g.lda_global_n(N3, c.ndoc), gn3)
    assert np.isfinite(N3).all() and (N3[~c.isolated] > 0).all()


@pytest.mark.parametrize("name", ["A1", "C"])
def test_dedicated_equals_generic(cases, name):
    c = cases[name]
    (Nd, gd), (Ng, gg) = three_iterations(c, 0), three_iterations(c, 1)
    assert same_bits(Nd, Ng) and same_bits(gd, gg)


@pytest.mark.parametrize("force", FORMS)
@pytest.mark.parametrize("name", ["A1", "B", "C"])
def test_loglik(cases, name, force):
    c = cases[name]
    N3, gn3 = three_iterations(c, 0)
    ref = c.memo("loglik", lambda: loglik(c.to_dev(N3), gn3, c.adj_out, ETA, c.nterms)[c.dov])
    c.set_form(force)
    total, tl = c.g.lda_loglik(N3, c.ndoc, c.nterms, ETA)
    nz = ref != 0
    print("%s force_ordered=%d: largest relative deviation of token_loglik %.3g" % (name, force, np.max(np.abs(tl[nz] - ref[nz]) / np.abs(ref[nz]))))
    np.testing.assert_allclose(tl, ref, rtol=1e-6, atol=0)
    assert (tl[: c.ndoc] == 0).all()
    exact = math.fsum(ref)
    assert abs(total - exact) <= 1e-6 * abs(exact)


def test_refusals(cases):
    import ctypes as C
    c = cases["A1"]
    api = c.api
    L = api._lib.lib()
    st = c.g._lda_to_device(c.ref_init(), c.ndoc)
    before = st.clone()
    it = C.c_int(0)
    out = (C.c_double * 20)()
    assert L.gm_run_lda(c.g.h, st.data_ptr(), 7, ALPHA, ETA, 60.0, 1, C.byref(it), None, None) == 4  # GM_ERR_UNSUPPORTED
    assert b"fixed menu" in L.gm_last_error()
    assert L.gm_run_lda(c.g.h, st.data_ptr(), 20, ALPHA, ETA, 60.0, 0, C.byref(it), None, None) == 1  # GM_ERR_INVALID
    assert L.gm_run_lda_init(c.g.h, st.data_ptr(), 7, None) == 4
    assert L.gm_lda_global_n(c.g.h, st.data_ptr(), 7, out, None) == 4
    assert (st == before).all()
    ndoc, nterms, s, d, v = corpus_a()
    g_out = api.Graph(ndoc + nterms, s, d, v, directions=api.GM_DIR_OUT)
    st2 = g_out._lda_to_device(c.ref_init(), ndoc)
    assert L.gm_run_lda(g_out.h, st2.data_ptr(), 20, ALPHA, ETA, 60.0, 1, C.byref(it), None, None) == 4
    assert b"both directions" in L.gm_last_error()
    with pytest.raises(api._lib.GMError):
        g_out.lda(c.ref_init(), ndoc, nterms, ALPHA, ETA, 1)
