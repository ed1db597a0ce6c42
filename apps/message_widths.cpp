// message_widths.cpp -- message, reduction, vertex-property and edge types that are NOT four bytes wide, on a graph with every row class.
//
// The engine is generic in T (message), U (reduced message), V (vertex property) and E (edge value); much of kernels.hpp / engine.hpp exists
// only for other widths than four bytes (the LDS staging of 1- and 2-byte messages in the row-blocks, the giant-row strategies by sizeof(U),
// the padded (id, message) entries of the list steps, the edge-value gates of the sweep / blocked stream / tiles).  Nine type shapes run
// here, each against a host restatement of run_graph_program: the active vertices send, every destination folds its present messages in
// stored order (ascending native id of the source; the first term initialises, later terms go through the program's own reduce_function),
// apply runs where a message arrived, a vertex is active when its property changed.  Every vertex property is compared byte for byte.
//
//   1  bool -> int            V {unsigned order; int pending}   E int     a += b      undeclared, and declared REDUCE_COMMUTATIVE
//   2  uchar -> uchar         V unsigned char                   E uchar   min         undeclared, and declared REDUCE_COMMUTATIVE
//   3  ushort -> ushort       V {ushort seen; ushort from}      E int     a = b       undeclared, and declared REDUCE_LAST
//   4  uchar -> ull           V unsigned long long              E int     a += b      ALL_VERTICES, 3 iterations
//   5  double -> double       V {double a; double b; int k}     E double  a += b      ALL_VERTICES x 2; ACTIVE_ONLY (every third vertex) x 3
//   6  float -> double        V double                          E float   a += b      ALL_VERTICES, 2 iterations
//   7  3 bytes -> 3 bytes     V int                             E int     add / xor / last by field, ALL_VERTICES, 1 iteration
//   8  12 bytes -> 12 bytes   V = the same {float; int; int}    E int     add / add / last, ACTIVE_ONLY (every second vertex), 2 iterations
//   9  int -> int             V int                             E uchar   a += b      ALL_VERTICES, 2 iterations: 4-byte messages and sums, which
//                                                                                       the sweep takes, over edge values it does not carry
//
// The graph (n = 60000): vertices 1..16 have exactly 20000, 8193, 8192, 4097, 4096, 1025, 1024, 300, 129, 128, 65, 64, 63, 2, 1, 0
// in-edges -- with the giant threshold at 4096 that is giant rows of five, three, two and two 4096-product pieces, the largest wave row, rows on
// both sides of GM_LONG_MID and of GM_SHORT_ROW -- from distinct sources, except that 50 of vertex 8's 300 in-edges are duplicates; the other
// vertices lie on a ring 17 -> 18 -> ... -> n -> 17 and receive 3n random edges (which may repeat).  The same (source, destination) list is
// built once per edge type; an edge's value is a hash of its end points, so duplicated edges carry equal values.
//
// One line per case: "<case>: <bad> of <n> vertices differ ..."; "WIDTHS PASS" and exit status 0 only when no vertex differs anywhere.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "GraphMatRuntime.h"

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) { printf("CHECK failed: %s (line %d)\n", #cond, __LINE__); failures++; } \
  } while (0)

static const int kN = 60000, kHubs = 16;
static const int kHubDegree[kHubs] = {20000, 8193, 8192, 4097, 4096, 1025, 1024, 300, 129, 128, 65, 64, 63, 2, 1, 0};

static inline unsigned mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
static inline unsigned edge_hash(int src, int dst) { return mix32((unsigned)src * 0x9E3779B1u ^ mix32((unsigned)dst)); }

// ---- vertex properties and messages --------------------------------------------------------------------------------------------------
struct Pending {  // case 1
  unsigned order;
  int pending;
  bool operator!=(const Pending& o) const { return order != o.order || pending != o.pending; }
  friend std::ostream& operator<<(std::ostream& os, const Pending& v) { return os << v.order; }
};
struct Seen {  // case 3
  unsigned short seen, from;
  bool operator!=(const Seen& o) const { return seen != o.seen || from != o.from; }
  friend std::ostream& operator<<(std::ostream& os, const Seen& v) { return os << v.from; }
};
struct Wide {  // case 5: 24 bytes, four of them padding
  double a, b;
  int k;
  bool operator!=(const Wide& o) const { return a != o.a || b != o.b || k != o.k; }
  friend std::ostream& operator<<(std::ostream& os, const Wide& v) { return os << v.a; }
};
struct Tri {  // case 7: three bytes, alignment 1
  unsigned char a, b, c;
};
static_assert(sizeof(Tri) == 3 && alignof(Tri) == 1, "a 3-byte message");
struct Tally {  // case 8: 12 bytes
  float s;
  int n, last;
  bool operator!=(const Tally& o) const { return s != o.s || n != o.n || last != o.last; }
  friend std::ostream& operator<<(std::ostream& os, const Tally& v) { return os << v.s; }
};
static_assert(sizeof(Pending) == 8 && sizeof(Seen) == 4 && sizeof(Wide) == 24 && sizeof(Tally) == 12, "the widths this program is about");

// byte-for-byte equality of two vertex properties (Wide: of its fields -- the padding behind k belongs to nobody)
template <class V>
static bool same_bytes(const V& a, const V& b) { return memcmp(&a, &b, sizeof(V)) == 0; }
static bool same_bytes(const Wide& a, const Wide& b) { return memcmp(&a.a, &b.a, 8) == 0 && memcmp(&a.b, &b.b, 8) == 0 && a.k == b.k; }

// ---- the programs ----------------------------------------------------------------------------------------------------------------------
// 1: every active vertex says whether it is ready (nothing pending); a destination counts the ready ones among its present senders, takes
// them off its own pending count and notes when (a counter that do_every_iteration advances).  1-byte messages, 4-byte sums.
template <int DECLARED>
class Ready : public GraphMat::GraphProgram<bool, int, Pending> {
 public:
  unsigned stamp;
  Ready() : stamp(1) { this->activity = GraphMat::ACTIVE_ONLY; this->process_message_requires_vertexprop = false; }
  bool send_message(const Pending& v, bool& m) const { m = v.pending == 0; return true; }
  void process_message(const bool& m, const int, const Pending&, int& r) const { r = m ? 1 : 0; }
  void reduce_function(int& a, const int& b) const { a += b; }
  void apply(const int& y, Pending& v) {
    if (y > 0) { v.pending -= y; v.order = stamp; }
  }
  void do_every_iteration(int) { stamp++; }
};
// 2: saturating 8-bit distances over 8-bit edge weights
template <int DECLARED>
class ByteDist : public GraphMat::GraphProgram<unsigned char, unsigned char, unsigned char, unsigned char> {
 public:
  ByteDist() { this->activity = GraphMat::ACTIVE_ONLY; this->process_message_requires_vertexprop = false; }
  bool send_message(const unsigned char& v, unsigned char& m) const { m = v; return true; }
  void process_message(const unsigned char& m, const unsigned char e, const unsigned char&, unsigned char& r) const {
    const int s = (int)m + (int)e;
    r = (unsigned char)(s > 255 ? 255 : s);
  }
  void reduce_function(unsigned char& a, const unsigned char& b) const { a = b < a ? b : a; }
  void apply(const unsigned char& y, unsigned char& v) { if (y < v) v = y; }
};
// 3: the last writer of a 16-bit tag: a vertex that is reached keeps the tag of its last present sender in stored order
template <int DECLARED>
class LastTag : public GraphMat::GraphProgram<unsigned short, unsigned short, Seen> {
 public:
  LastTag() { this->activity = GraphMat::ACTIVE_ONLY; this->process_message_requires_vertexprop = false; }
  bool send_message(const Seen& v, unsigned short& m) const { m = (unsigned short)((v.from * 40503u + v.seen * 0x9E37u + 0x1234u) >> 3); return true; }
  void process_message(const unsigned short& m, const int, const Seen&, unsigned short& r) const { r = m; }
  void reduce_function(unsigned short& a, const unsigned short& b) const { a = b; }
  void apply(const unsigned short& y, Seen& v) {
    if (v.seen == 0) { v.seen = 1; v.from = y; }
  }
};
// 4: 1-byte messages summed into 8 bytes
class ByteSum : public GraphMat::GraphProgram<unsigned char, unsigned long long, unsigned long long> {
 public:
  ByteSum() { this->activity = GraphMat::ALL_VERTICES; this->process_message_requires_vertexprop = false; }
  bool send_message(const unsigned long long& v, unsigned char& m) const { m = (unsigned char)((v * 0x9E3779B97F4A7C15ull) >> 56); return true; }
  void process_message(const unsigned char& m, const int e, const unsigned long long&, unsigned long long& r) const { r = (unsigned long long)m * (unsigned long long)e; }
  void reduce_function(unsigned long long& a, const unsigned long long& b) const { a += b; }
  void apply(const unsigned long long& y, unsigned long long& v) { v = v * 6364136223846793005ull + y; }
};
// 5: fp64 sums over fp64 edge values into a 24-byte property
class WideSum : public GraphMat::GraphProgram<double, double, Wide, double> {
 public:
  explicit WideSum(GraphMat::activity_type a) { this->activity = a; this->process_message_requires_vertexprop = false; }
  bool send_message(const Wide& v, double& m) const { m = v.a; return true; }
  void process_message(const double& m, const double e, const Wide&, double& r) const { r = m * e; }
  void reduce_function(double& a, const double& b) const { a += b; }
  void apply(const double& y, Wide& v) {
    v.b = y;
    const double keep = v.a * 0.5;
    v.a = y * 0.001 + keep;
    v.k++;
  }
};
// 6: fp32 messages and edge values, fp64 sums
class MixedSum : public GraphMat::GraphProgram<float, double, double, float> {
 public:
  MixedSum() { this->activity = GraphMat::ALL_VERTICES; this->process_message_requires_vertexprop = false; }
  bool send_message(const double& v, float& m) const { m = (float)v; return true; }
  void process_message(const float& m, const float e, const double&, double& r) const { r = (double)m * (double)e; }
  void reduce_function(double& a, const double& b) const { a += b; }
  void apply(const double& y, double& v) {
    const double keep = v * 0.5;
    v = y * 0.001 + keep;
  }
};
// 7: a 3-byte message and reduction: wrapping add, xor, last
class TriFold : public GraphMat::GraphProgram<Tri, Tri, int> {
 public:
  TriFold() { this->activity = GraphMat::ALL_VERTICES; this->process_message_requires_vertexprop = false; }
  bool send_message(const int& v, Tri& m) const { m.a = (unsigned char)v; m.b = (unsigned char)(v >> 8); m.c = (unsigned char)(v >> 16); return true; }
  void process_message(const Tri& m, const int e, const int&, Tri& r) const { r = m; r.a = (unsigned char)(m.a + e); }
  void reduce_function(Tri& a, const Tri& b) const { a.a = (unsigned char)(a.a + b.a); a.b ^= b.b; a.c = b.c; }
  void apply(const Tri& y, int& v) { v = (int)y.a | ((int)y.b << 8) | ((int)y.c << 16) | 0x01000000; }
};
// 8: a 12-byte message, reduction and property: float sum, count, last
class TallyFold : public GraphMat::GraphProgram<Tally, Tally, Tally> {
 public:
  TallyFold() { this->activity = GraphMat::ACTIVE_ONLY; this->process_message_requires_vertexprop = false; }
  bool send_message(const Tally& v, Tally& m) const { m = v; return true; }
  void process_message(const Tally& m, const int e, const Tally&, Tally& r) const { r = m; r.n = m.n * e; }
  void reduce_function(Tally& a, const Tally& b) const { a.s += b.s; a.n += b.n; a.last = b.last; }
  void apply(const Tally& y, Tally& v) { v.s = y.s * 0.01f; v.n = y.n % 1000 + 1; v.last = y.last; }
};
// 9: 4-byte messages and sums over 1-byte edge values
class ByteWeighted : public GraphMat::GraphProgram<int, int, int, unsigned char> {
 public:
  ByteWeighted() { this->activity = GraphMat::ALL_VERTICES; this->process_message_requires_vertexprop = false; }
  bool send_message(const int& v, int& m) const { m = v & 0xffff; return true; }
  void process_message(const int& m, const unsigned char e, const int&, int& r) const { r = m * (int)e; }
  void reduce_function(int& a, const int& b) const { a += b; }
  void apply(const int& y, int& v) { v = (int)((unsigned)v * 1103515245u + (unsigned)y); }
};
namespace GraphMat {
template <> struct program_traits<Ready<1> > { static constexpr reduce_kind reduce = REDUCE_COMMUTATIVE; };
template <> struct program_traits<ByteDist<1> > { static constexpr reduce_kind reduce = REDUCE_COMMUTATIVE; };
template <> struct program_traits<LastTag<1> > { static constexpr reduce_kind reduce = REDUCE_LAST; };
}  // namespace GraphMat

// ---- the graph --------------------------------------------------------------------------------------------------------------------------
struct Link { int src, dst; };
static std::vector<Link> build_links() {
  std::vector<Link> ed;
  unsigned st = 2463534242u;
  auto next = [&]() { st = st * 1664525u + 1013904223u; return st >> 8; };
  const int rest = kN - kHubs;  // 59984 = 2^4 * 23 * 163: a stride of 7919 visits every vertex of 17..n before it repeats
  for (int h = 0; h < kHubs; h++) {
    const int distinct = h == 7 ? kHubDegree[h] - 50 : kHubDegree[h];
    const unsigned start = next() % (unsigned)rest;
    for (int k = 0; k < distinct; k++) ed.push_back(Link{kHubs + 1 + (int)((start + (unsigned long long)k * 7919ull) % (unsigned long long)rest), 1 + h});
    for (int k = 0; k < kHubDegree[h] - distinct; k++) ed.push_back(Link{kHubs + 1 + (int)((start + (unsigned long long)(3 * k) * 7919ull) % (unsigned long long)rest), 1 + h});
  }
  for (int i = 0; i < rest; i++) ed.push_back(Link{kHubs + 1 + i, kHubs + 1 + (i + 1) % rest});
  for (int i = 0; i < 3 * kN; i++) {
    const int s = 1 + (int)(next() % (unsigned)kN), d = kHubs + 1 + (int)(next() % (unsigned)rest);
    ed.push_back(Link{s, d});
  }
  return ed;
}

template <class E, class W>
static std::vector<GraphMat::edge_t<E> > weighted(const std::vector<Link>& links, W weight) {
  std::vector<GraphMat::edge_t<E> > ed;
  ed.reserve(links.size());
  for (const Link& l : links) ed.push_back(GraphMat::edge_t<E>(l.src, l.dst, weight(edge_hash(l.src, l.dst))));
  return ed;
}

template <class V, class E>
static void read_graph(GraphMat::Graph<V, E>& G, const std::vector<GraphMat::edge_t<E> >& ed) {
  GraphMat::edgelist_t<E> L(kN, kN, (int)ed.size());
  std::copy(ed.begin(), ed.end(), L.edges);
  G.ReadEdgelist(L);
  L.clear();
}

// in-edges of every vertex in stored order: (source, edge value), ascending native id of the source (Graph.h renumbers the vertices)
template <class E>
struct InLists {
  std::vector<std::vector<std::pair<int, E> > > in;
  template <class V>
  InLists(const GraphMat::Graph<V, E>& G, const std::vector<GraphMat::edge_t<E> >& ed) : in(kN + 1) {
    std::vector<int> nat(kN + 1);
    for (int v = 1; v <= kN; v++) nat[v] = G.vertexToNative(v, G.tiles_per_dim, G.nvertices);
    for (const auto& e : ed) in[e.dst].push_back(std::make_pair(e.src, e.val));
    for (int v = 1; v <= kN; v++)
      std::stable_sort(in[v].begin(), in[v].end(), [&](const std::pair<int, E>& a, const std::pair<int, E>& b) { return nat[a.first] < nat[b.first]; });
  }
};

// ---- the host restatement of run_graph_program (no device, no library: the program's methods and plain loops) -----------------------------
template <class P, class T, class U, class V, class E>
static int host_run(P& prog, const InLists<E>& g, std::vector<V>& vp, std::vector<char>& act, bool all_vertices, int iterations) {
  std::unique_ptr<T[]> x(new T[kN + 1]());  // (not a std::vector: T may be bool)
  std::vector<char> next_act(kN + 1);
  int it = 0;
  while (true) {
    if (all_vertices) std::fill(act.begin(), act.end(), 1);
    for (int v = 1; v <= kN; v++)
      if (act[v]) prog.send_message(vp[v], x[v]);
    std::fill(next_act.begin(), next_act.end(), 0);
    bool any = false;
    std::vector<V> out(vp);
    for (int v = 1; v <= kN; v++) {
      bool has = false;
      U acc;
      for (const auto& se : g.in[v]) {
        if (!act[se.first]) continue;
        U r;
        prog.process_message(x[se.first], se.second, vp[v], r);
        if (has) prog.reduce_function(acc, r); else { acc = r; has = true; }
      }
      if (!has) continue;
      prog.apply(acc, out[v]);
      if (out[v] != vp[v]) { next_act[v] = 1; any = true; }
    }
    vp.swap(out);
    act.swap(next_act);
    prog.do_every_iteration(it);
    it++;
    if (iterations > 0 ? it == iterations : !any) break;
  }
  return it;
}

struct CaseResult { const char* name; int strategy; };
static std::vector<CaseResult> ran;

// one case: the same start on the host and on the device, then every vertex property byte for byte
template <class P, class V, class E>
static void run_case(const char* name, P host_prog, P dev_prog, GraphMat::Graph<V, E>& G, const InLists<E>& lists, const std::vector<V>& start,
                     const std::vector<char>& active, int iterations) {
  typedef typename P::message_type T;
  typedef typename P::message_reduction_type U;
  printf("== %s\n", name);
  {
    int tiles = 1;
    gm_sweep_t sw;
    memset(&sw, 0, sizeof(sw));
    gm_graph_tiles(G.A, GM_DIR_OUT, &tiles);
    if (gm_graph_sweep(G.A, &sw) != 0) memset(&sw, 0, sizeof(sw));
    printf("   graph: %d column tiles, sweep of %d rows (value bytes %d)\n", tiles, (int)sw.nrows, sw.nrows > 0 ? (int)sw.val_bytes : 0);
  }
  fflush(stdout);
  const bool all_vertices = host_prog.getActivity() == GraphMat::ALL_VERTICES;
  std::vector<V> want(start);
  std::vector<char> act(active);
  const int host_its = host_run<P, T, U, V, E>(host_prog, lists, want, act, all_vertices, iterations);
  G.setAllInactive();
  for (int v = 1; v <= kN; v++) {
    G.setVertexproperty(v, start[v]);
    if (all_vertices || active[v]) G.setActive(v);
  }
  ran.push_back(CaseResult{name, GraphMat::detail::reduce_kind_of<P, U>(&dev_prog)});
  GraphMat::run_graph_program(&dev_prog, G, iterations > 0 ? iterations : GraphMat::UNTIL_CONVERGENCE);
  int bad = 0, first = 0;
  for (int v = 1; v <= kN; v++) {
    const V got = G.getVertexproperty(v);
    if (!same_bytes(got, want[v])) { if (!bad) first = v; bad++; }
  }
  printf("%s: %d of %d vertices differ from the host's ordered fold after %d iterations", name, bad, kN, host_its);
  if (bad) printf(" (first: vertex %d, %d in-edges)", first, (int)lists.in[first].size());
  printf("\n");
  fflush(stdout);
  if (bad) failures++;
}

static double mixed_value(int v) { return 1.0 / (double)(v % 97 + 1) + (double)(v % 13) * 0.37; }  // non-dyadic, mixed magnitudes: sums round at every step

int main(int argc, char** argv) {
  MPI_Init(&argc, &argv);
  const std::vector<Link> links = build_links();
  std::vector<int> indeg(kN + 1, 0);
  for (const Link& l : links) indeg[l.dst]++;
  for (int h = 0; h < kHubs; h++) CHECK(indeg[1 + h] == kHubDegree[h]);
  const std::vector<char> nobody(kN + 1, 0);
  const auto int_edges = weighted<int>(links, [](unsigned h) { return 1 + (int)(h % 3u); });

  {  // ---- 1: bool -> int
    GraphMat::Graph<Pending, int> G;
    read_graph(G, int_edges);
    gm_csr_t ca;
    CHECK(gm_graph_csr(G.A, GM_DIR_OUT, &ca) == 0);
    printf("%d vertices, %d edges: %d giant rows in %d pieces, %d wave rows (%d long), %d row-blocks\n", kN, (int)links.size(), ca.ngiant, ca.ngchunk, ca.nmid,
           ca.nmid_long, ca.nblk);
    CHECK(ca.ngiant >= 3);
    CHECK(ca.nmid > 0);
    CHECK(ca.nmid_long > 0);
    CHECK(ca.nblk > 0);
    const InLists<int> lists(G, int_edges);
    // every vertex starts with its in-degree pending, except that every third vertex behind the hubs has been released (nothing pending):
    // the first iteration's messages are a mix of true and false on every row, later ones come from the few vertices that just changed
    std::vector<Pending> start(kN + 1);
    std::vector<char> everybody(kN + 1, 1);
    for (int v = 1; v <= kN; v++) start[v] = Pending{0u, (v > kHubs && v % 3 == 0) ? 0 : indeg[v]};
    run_case("1 bool->int", Ready<0>(), Ready<0>(), G, lists, start, everybody, -1);
    run_case("1 bool->int, declared commutative", Ready<1>(), Ready<1>(), G, lists, start, everybody, -1);
  }
  {  // ---- 2: unsigned char everywhere
    const auto ed = weighted<unsigned char>(links, [](unsigned h) { return (unsigned char)(1u + h % 9u); });
    GraphMat::Graph<unsigned char, unsigned char> G;
    read_graph(G, ed);
    const InLists<unsigned char> lists(G, ed);
    // plain distances from the source first (host, integers), then the source starts so high that half of the reachable vertices saturate
    const int source = 17 + 4242;
    std::vector<int> d(kN + 1, 1 << 30);
    d[source] = 0;
    for (bool moved = true; moved;) {
      moved = false;
      for (const auto& e : ed)
        if (d[e.src] < (1 << 30) && d[e.src] + (int)e.val < d[e.dst]) { d[e.dst] = d[e.src] + (int)e.val; moved = true; }
    }
    std::vector<int> reach;
    for (int v = 1; v <= kN; v++) if (d[v] < (1 << 30)) reach.push_back(d[v]);
    std::sort(reach.begin(), reach.end());
    const int median = reach[reach.size() / 2];
    CHECK(reach.size() > (size_t)kN / 2 && median > 0 && median < 200);
    const int base = 254 - median;
    int below = 0, saturated = 0;
    for (int x : reach) { if (base + x < 255) below++; else saturated++; }
    printf("case 2: source %d starts at %d: %d vertices end below 255, %d reachable ones saturate\n", source, base, below, saturated);
    CHECK(below > 1000 && saturated > 1000);
    std::vector<unsigned char> start(kN + 1, (unsigned char)255);
    start[source] = (unsigned char)base;
    std::vector<char> active(nobody);
    active[source] = 1;
    run_case("2 uchar->uchar", ByteDist<0>(), ByteDist<0>(), G, lists, start, active, -1);
    run_case("2 uchar->uchar, declared commutative", ByteDist<1>(), ByteDist<1>(), G, lists, start, active, -1);
  }
  {  // ---- 3: unsigned short, a = b
    GraphMat::Graph<Seen, int> G;
    read_graph(G, int_edges);
    const InLists<int> lists(G, int_edges);
    const int source = 17 + 977;
    std::vector<Seen> start(kN + 1);
    for (int v = 1; v <= kN; v++) start[v] = Seen{0, (unsigned short)(mix32((unsigned)v) >> 7)};
    start[source].seen = 1;
    std::vector<char> active(nobody);
    active[source] = 1;
    run_case("3 ushort->ushort", LastTag<0>(), LastTag<0>(), G, lists, start, active, -1);
    run_case("3 ushort->ushort, declared last", LastTag<1>(), LastTag<1>(), G, lists, start, active, -1);
  }
  {  // ---- 4: unsigned char -> unsigned long long
    GraphMat::Graph<unsigned long long, int> G;
    read_graph(G, int_edges);
    const InLists<int> lists(G, int_edges);
    std::vector<unsigned long long> start(kN + 1);
    for (int v = 1; v <= kN; v++) start[v] = ((unsigned long long)mix32((unsigned)v) << 32) | mix32((unsigned)v + 77u);
    run_case("4 uchar->ull", ByteSum(), ByteSum(), G, lists, start, nobody, 3);
  }
  {  // ---- 5: double, 24-byte property, double edge values
    const auto ed = weighted<double>(links, [](unsigned h) { return 1.0 + (double)(h % 7u) / 8.0; });
    GraphMat::Graph<Wide, double> G;
    read_graph(G, ed);
    const InLists<double> lists(G, ed);
    std::vector<Wide> start(kN + 1);
    for (int v = 1; v <= kN; v++) {
      memset(&start[v], 0, sizeof(Wide));
      start[v].a = mixed_value(v);
      start[v].k = v % 5;
    }
    run_case("5a double->double, all vertices", WideSum(GraphMat::ALL_VERTICES), WideSum(GraphMat::ALL_VERTICES), G, lists, start, nobody, 2);
    std::vector<char> third(nobody);
    for (int v = 1; v <= kN; v += 3) third[v] = 1;
    run_case("5b double->double, active only", WideSum(GraphMat::ACTIVE_ONLY), WideSum(GraphMat::ACTIVE_ONLY), G, lists, start, third, 3);
  }
  {  // ---- 6: float -> double over float edge values
    const auto ed = weighted<float>(links, [](unsigned h) { return 1.0f + (float)(h % 7u) / 8.0f; });
    GraphMat::Graph<double, float> G;
    read_graph(G, ed);
    const InLists<float> lists(G, ed);
    std::vector<double> start(kN + 1);
    for (int v = 1; v <= kN; v++) start[v] = mixed_value(v);
    run_case("6 float->double", MixedSum(), MixedSum(), G, lists, start, nobody, 2);
  }
  {  // ---- 7: three bytes
    GraphMat::Graph<int, int> G;
    read_graph(G, int_edges);
    const InLists<int> lists(G, int_edges);
    std::vector<int> start(kN + 1);
    for (int v = 1; v <= kN; v++) start[v] = (int)(mix32((unsigned)v * 3u + 1u) & 0x00ffffffu);
    run_case("7 3 bytes->3 bytes", TriFold(), TriFold(), G, lists, start, nobody, 1);
  }
  {  // ---- 8: twelve bytes
    GraphMat::Graph<Tally, int> G;
    read_graph(G, int_edges);
    const InLists<int> lists(G, int_edges);
    std::vector<Tally> start(kN + 1);
    for (int v = 1; v <= kN; v++) start[v] = Tally{(float)mixed_value(v), 1 + v % 7, v};
    std::vector<char> half(nobody);
    for (int v = 1; v <= kN; v += 2) half[v] = 1;
    run_case("8 12 bytes->12 bytes", TallyFold(), TallyFold(), G, lists, start, half, 2);
  }
  {  // ---- 9: four bytes over unsigned char edge values
    const auto ed = weighted<unsigned char>(links, [](unsigned h) { return (unsigned char)(1u + h % 9u); });
    GraphMat::Graph<int, unsigned char> G;
    read_graph(G, ed);
    const InLists<unsigned char> lists(G, ed);
    std::vector<int> start(kN + 1);
    for (int v = 1; v <= kN; v++) start[v] = (int)mix32((unsigned)v + 99u);
    run_case("9 int->int over uchar edges", ByteWeighted(), ByteWeighted(), G, lists, start, nobody, 2);
  }
  for (const CaseResult& c : ran) printf("reduce strategy of case %s: %d\n", c.name, c.strategy);
  printf(failures == 0 ? "WIDTHS PASS\n" : "WIDTHS FAIL (%d)\n", failures);
  MPI_Finalize();
  return failures == 0 ? 0 : 1;
}
