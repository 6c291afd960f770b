// Ordering, symbolic factorisation and launch tables of the level-scheduled tile Cholesky (host code only; see chol_plan.h).
#include "chol_plan.h"
#include <thread>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>

#include "../../include/mpsfm_hip_debug.h"
#include "host_parts.h"

namespace mpsfm {
namespace {

constexpr int kTileCols = 32;    // every segment but the last ends on a tile boundary (padding columns)
constexpr int kMinLeaf = 32;     // no dissection below this many cameras
constexpr int kMinBfsLevels = 5;
constexpr int kMinCutCams = 64;   // ... and on graphs of at least this many cameras (twelve tile columns)
constexpr int kMinCutLevels = 8;  // the window-separator orders are tried on chains of at least this many levels
constexpr int kMinCutGain = 2;    // ... and taken for at least this many levels less: one level (~8 us per iteration) is within what
                                  // their padding columns and extra products may cost, two are not
constexpr int kFitWork = 2;        // refit: cameras of the parts laid out anew, in graphs (2: one half of an orbit, all the way down)
constexpr int kFastPanelSrc = 2, kFastTrailSrc = 4;  // sources the unrolled forms of k_chol_level take (dense_chol.hip: kPanelBatch, kTrailBatch)
constexpr double kMaxPlanProducts = 3.0e6;  // tile products beyond which no item table is built (tens of MB of tables, seconds to build)

using Mask = std::vector<uint64_t>;

struct Sub {  // breadth-first search inside a node subset
  const CamGraph& g;
  Mask in, seen;
  explicit Sub(const CamGraph& g_) : g(g_), in((size_t)g_.words, 0), seen((size_t)g_.words, 0) {}
  void set_nodes(const std::vector<int>& nodes) {
    std::fill(in.begin(), in.end(), 0);
    for (int v : nodes) in[(size_t)(v >> 6)] |= 1ull << (v & 63);
  }
  int degree(int v) const {
    int d = 0;
    const uint64_t* r = g.row(v);
    for (int w = 0; w < g.words; ++w) d += __builtin_popcountll(r[w] & in[(size_t)w]);
    return d;
  }
  // order: nodes by level, level_start: offsets (last entry = size).  Only nodes of `in` that are not in `seen` yet.
  void bfs(int start, std::vector<int>& order, std::vector<int>& level_start, bool reset_seen) {
    if (reset_seen) std::fill(seen.begin(), seen.end(), 0);
    order.clear(); level_start.clear();
    order.push_back(start); seen[(size_t)(start >> 6)] |= 1ull << (start & 63);
    level_start.push_back(0);
    size_t lo = 0;
    while (lo < order.size()) {
      const size_t hi = order.size();
      for (size_t q = lo; q < hi; ++q) {
        const uint64_t* r = g.row(order[q]);
        for (int w = 0; w < g.words; ++w) {
          uint64_t m = r[w] & in[(size_t)w] & ~seen[(size_t)w];
          seen[(size_t)w] |= m;
          while (m) { order.push_back(w * 64 + __builtin_ctzll(m)); m &= m - 1; }
        }
      }
      lo = hi;
      if (order.size() > hi) level_start.push_back((int)hi);
    }
    level_start.push_back((int)order.size());
  }
};

void components(Sub& S, const std::vector<int>& nodes, std::vector<std::vector<int>>& comps) {
  comps.clear();
  S.set_nodes(nodes);
  std::fill(S.seen.begin(), S.seen.end(), 0);
  std::vector<int> order, ls;
  for (int v : nodes) {
    if ((S.seen[(size_t)(v >> 6)] >> (v & 63)) & 1) continue;
    S.bfs(v, order, ls, false);
    comps.push_back(order);
    std::sort(comps.back().begin(), comps.back().end());
  }
}

// a node far from the "middle" of a connected subset: repeated BFS from a lowest-degree node of the last level
int pseudo_peripheral(Sub& S, const std::vector<int>& nodes, std::vector<int>& order, std::vector<int>& ls) {
  S.set_nodes(nodes);
  int s = nodes[0], best = 1 << 30;
  for (int v : nodes) { const int d = S.degree(v); if (d < best) { best = d; s = v; } }
  int depth = -1;
  for (int it = 0; it < 8; ++it) {
    S.bfs(s, order, ls, true);
    const int nl = (int)ls.size() - 1;
    if (nl <= depth) break;
    depth = nl;
    int cand = s, bd = 1 << 30;
    for (int q = ls[(size_t)nl - 1]; q < ls[(size_t)nl]; ++q) { const int d = S.degree(order[(size_t)q]); if (d < bd) { bd = d; cand = order[(size_t)q]; } }
    if (cand == s) break;
    s = cand;
  }
  S.bfs(s, order, ls, true);
  return s;
}

// reverse Cuthill-McKee of a subset (every component from a pseudo-peripheral node)
void rcm(Sub& S, const std::vector<int>& nodes, std::vector<int>& out) {
  std::vector<std::vector<int>> comps;
  components(S, nodes, comps);
  std::vector<int> order, ls;
  for (const auto& c : comps) {
    pseudo_peripheral(S, c, order, ls);
    out.insert(out.end(), order.rbegin(), order.rend());
  }
}

struct Seg { std::vector<int> cams; std::vector<int> child; };

int dissect(Sub& S, std::vector<Seg>& tree, const std::vector<int>& nodes, int depth) {
  const int me = (int)tree.size();
  tree.emplace_back();
  std::vector<std::vector<int>> comps;
  components(S, nodes, comps);
  if (comps.size() > 1) {  // independent parts: an empty separator above them
    for (const auto& c : comps) { const int ch = dissect(S, tree, c, depth); tree[(size_t)me].child.push_back(ch); }
    return me;
  }
  std::vector<int> order, ls;
  if (depth > 0 && (int)nodes.size() >= kMinLeaf) {
    pseudo_peripheral(S, nodes, order, ls);
    const int nl = (int)ls.size() - 1;
    if (nl >= kMinBfsLevels) {
      // the level whose removal leaves the smallest larger side plus itself
      int bm = -1; long best = 1L << 60;
      for (int m = 1; m < nl - 1; ++m) {
        const long a = ls[(size_t)m], b = (long)order.size() - ls[(size_t)m + 1], s = ls[(size_t)m + 1] - ls[(size_t)m];
        const long cost = std::max(a, b) + s;
        if (cost < best) { best = cost; bm = m; }
      }
      if (bm > 0) {
        std::vector<int> A(order.begin(), order.begin() + ls[(size_t)bm]), B(order.begin() + ls[(size_t)bm + 1], order.end()),
            sep(order.begin() + ls[(size_t)bm], order.begin() + ls[(size_t)bm + 1]);
        // cameras of the level that see nothing beyond it are not needed in the separator: a level is as wide as the LONGEST
        // link out of the level before it, most cameras reach less far
        {
          S.set_nodes(B);
          std::vector<int> keep;
          for (int v : sep) { if (S.degree(v) > 0) keep.push_back(v); else A.push_back(v); }
          if (!keep.empty()) sep.swap(keep);
          else { for (size_t q = 0; q < sep.size(); ++q) A.pop_back(); }  // (a level without forward links cannot be a middle level)
        }
        std::sort(A.begin(), A.end()); std::sort(B.begin(), B.end()); std::sort(sep.begin(), sep.end());
        const int ca = dissect(S, tree, A, depth - 1);
        const int cb = dissect(S, tree, B, depth - 1);
        tree[(size_t)me].child = {ca, cb};
        rcm(S, sep, tree[(size_t)me].cams);
        return me;
      }
    }
  }
  rcm(S, nodes, tree[(size_t)me].cams);
  return me;
}

// Post-order flattening.  kSegEnd after every segment but the last: the next camera starts on a tile boundary (padding
// columns in between).  A segment that exceeds a whole number of tiles by a few cameras hands them to its parent instead
// (a separator stays one when it grows), so that its chain is a tile shorter.
constexpr int kSegEnd = -1;
void flatten(const std::vector<Seg>& tree, int node, bool is_root, int move_up, std::vector<int>& out, std::vector<int>& up) {
  std::vector<int> cams;
  for (int c : tree[(size_t)node].child) {
    std::vector<int> moved;
    flatten(tree, c, false, move_up, out, moved);
    cams.insert(cams.end(), moved.begin(), moved.end());
  }
  const std::vector<int>& own = tree[(size_t)node].cams;
  if (!is_root && own.empty()) { up = cams; return; }  // independent parts under an empty separator: what moved up keeps moving
  cams.insert(cams.end(), own.begin(), own.end());
  if (cams.empty()) return;
  if (!is_root) {
    const int k = (int)cams.size();
    const int whole = (6 * k) / kTileCols * kTileCols / 6;  // cameras that fit the whole tiles of the segment
    const int over = k - whole;
    if (over > 0 && over <= move_up && whole > 0 && (6 * k) % kTileCols != 0) {
      up.assign(cams.end() - over, cams.end());
      cams.resize((size_t)whole);
    }
  }
  out.insert(out.end(), cams.begin(), cams.end());
  if (!is_root) out.push_back(kSegEnd);
}

// slots and first columns of the ncams cameras of a segment tree
void slots_from_tree(const std::vector<Seg>& tree, int ncams, int move_up, std::vector<int32_t>& slot_of_nat, std::vector<int32_t>& col_of_slot, int& n_cols) {
  slot_of_nat.assign((size_t)ncams, -1);
  col_of_slot.assign((size_t)ncams, 0);
  std::vector<int> out, up;
  flatten(tree, 0, true, move_up, out, up);
  while (!out.empty() && out.back() == kSegEnd) out.pop_back();  // nothing follows the last segment
  int slot = 0, col = 0;
  for (int v : out) {
    if (v == kSegEnd) { col = (col + kTileCols - 1) / kTileCols * kTileCols; continue; }
    slot_of_nat[(size_t)v] = slot;
    col_of_slot[(size_t)slot] = col;
    ++slot; col += 6;
  }
  n_cols = col;
}

// ---- dissection by minimal window separators ------------------------------------------------------------------------------------
// dissect() cuts at whole breadth-first levels, balances in cameras and leaves parts below kMinLeaf alone.  Here a part is laid
// out as a linear arrangement (the breadth-first order from a pseudo-peripheral camera, forwards and backwards, and the caller's
// order) and cut by a WINDOW of it: with far[i] the last position adjacent to position i, the narrowest separator that starts
// at c is [c, max far[0 .. c) + 1) — no link passes over it.  Cuts are chosen and kept by the length of the chain in TILES.
inline int seg_tiles(int cams) { return (6 * cams + kTileCols - 1) / kTileCols; }

// Tile columns on the longest root-to-leaf path of a segment tree, the hand-over of flatten() included (up: cameras handed on).
// An upper bound of the levels of the real symbolic factorisation: a segment's tile columns need not be one chain.
int chain_tiles(const std::vector<Seg>& tree, int node, bool is_root, int move_up, int& up) {
  int k = 0, below = 0;
  for (int c : tree[(size_t)node].child) {
    int moved = 0;
    below = std::max(below, chain_tiles(tree, c, false, move_up, moved));
    k += moved;
  }
  up = 0;
  const int own = (int)tree[(size_t)node].cams.size();
  if (!is_root && own == 0) { up = k; return below; }
  k += own;
  if (k == 0) return below;
  if (!is_root) {
    const int whole = (6 * k) / kTileCols * kTileCols / 6, over = k - whole;
    if (over > 0 && over <= move_up && whole > 0 && (6 * k) % kTileCols != 0) { up = over; k = whole; }
  }
  return below + seg_tiles(k);
}

int tree_depth(const std::vector<Seg>& tree, int node) {  // separators above the deepest leaf
  int d = 0;
  for (int c : tree[(size_t)node].child) d = std::max(d, 1 + tree_depth(tree, c));
  return d;
}

struct WindowCut { int lo = 0, hi = 0; long cost = 1L << 60; int sep = 0, skew = 0; };  // separator [lo, hi) of the arrangement, trimmed sizes

// far[q] / near[q]: the last / first position of an arrangement adjacent to position q (q itself if none); pos: scratch of g.n entries
void reach_of(const CamGraph& g, const Mask& in, const std::vector<int>& arr, std::vector<int>& pos, std::vector<int>& far, std::vector<int>* near) {
  const int m = (int)arr.size();
  for (int q = 0; q < m; ++q) pos[(size_t)arr[(size_t)q]] = q;
  for (int q = 0; q < m; ++q) {
    int f = q, n = q;
    const uint64_t* r = g.row(arr[(size_t)q]);
    for (int w = 0; w < g.words; ++w) {
      uint64_t b = r[w] & in[(size_t)w];
      while (b) { const int p = pos[(size_t)(w * 64 + __builtin_ctzll(b))]; f = std::max(f, p); n = std::min(n, p); b &= b - 1; }
    }
    far[(size_t)q] = f;
    if (near) (*near)[(size_t)q] = n;
  }
}

// every window of an arrangement of m cameras given its far[]: visit(c, e, nl, ns, nr) with the separator [c, e) and the sizes of
// the left part, the separator and the right part once the window cameras that see nothing beyond the window have gone to the left
// near (optional): those of the rest that see nothing before the window are counted to the right part, as split_at_window() does
template <class Visit>
void windows_of(const std::vector<int>& far, const std::vector<int>* near, int m, Visit&& visit) {
  int reach = -1;  // max far[0 .. c)
  for (int c = 1; c < m; ++c) {
    reach = std::max(reach, far[(size_t)c - 1]);
    const int e = std::max(c, reach + 1);
    if (e >= m) break;  // reach only grows: no later window leaves a right part
    if (e == c) continue;  // (a connected part has no empty separator)
    int back = 0, front = 0;  // window cameras that see nothing beyond the window go to the left part
    for (int q = c; q < e; ++q) {
      if (far[(size_t)q] < e) ++back;
      else if (near && (*near)[(size_t)q] >= c) ++front;
    }
    const int nl = c + back, ns = e - c - back - front, nr = m - e + front;
    if (ns <= 0) continue;
    visit(c, e, nl, ns, nr);
  }
}

template <class Visit>
void for_each_window(const CamGraph& g, const Mask& in, const std::vector<int>& arr, std::vector<int>& pos, std::vector<int>& far, Visit&& visit) {
  reach_of(g, in, arr, pos, far, nullptr);
  windows_of(far, nullptr, (int)arr.size(), visit);
}

// the best window of one arrangement by the chain of ONE cut in tiles
void best_window(const CamGraph& g, const Mask& in, const std::vector<int>& arr, std::vector<int>& pos, std::vector<int>& far, WindowCut& best, int& best_arr, int arr_id) {
  for_each_window(g, in, arr, pos, far, [&](int c, int e, int nl, int ns, int nr) {
    const long cost = std::max(seg_tiles(nl), seg_tiles(nr)) + seg_tiles(ns);
    const int skew = std::abs(nl - nr);
    if (cost < best.cost || (cost == best.cost && (ns < best.sep || (ns == best.sep && skew < best.skew)))) {
      best.lo = c; best.hi = e; best.cost = cost; best.sep = ns; best.skew = skew; best_arr = arr_id;
    }
  });
}

using Tree = std::vector<Seg>;  // node 0 is the root
int graft(Tree& t, Tree&& sub) {  // appends a tree, returns where its root went
  const int off = (int)t.size();
  for (Seg& s : sub) {
    for (int& c : s.child) c += off;
    t.push_back(std::move(s));
  }
  return off;
}

// the three node sets of the window [lo, hi) of an arrangement: window cameras that see nothing on the right go
// to the left part, those that then see nothing on the left to the right one.  false: no separator is left, or nothing beside it
bool split_at_window(Sub& S, const std::vector<int>& ar, int lo, int hi, std::vector<int>& A, std::vector<int>& sep, std::vector<int>& B) {
  std::vector<int> keep, right;
  A.assign(ar.begin(), ar.begin() + lo); sep.assign(ar.begin() + lo, ar.begin() + hi); B.assign(ar.begin() + hi, ar.end());
  S.set_nodes(B);
  for (int v : sep) { if (S.degree(v) > 0) keep.push_back(v); else A.push_back(v); }
  sep.swap(keep); keep.clear();
  S.set_nodes(A);
  for (int v : sep) { if (S.degree(v) > 0) keep.push_back(v); else right.push_back(v); }
  if (keep.empty() || keep.size() >= ar.size()) return false;
  sep.swap(keep);
  B.insert(B.begin(), right.begin(), right.end());  // (all three in the order of the arrangement)
  return true;
}

Tree cut_dissect(Sub& S, const std::vector<int>& nodes, int move_up) {
  Tree t(1);
  std::vector<std::vector<int>> comps;
  components(S, nodes, comps);
  if (comps.size() > 1) {
    for (const auto& c : comps) { const int ch = graft(t, cut_dissect(S, c, move_up)); t[0].child.push_back(ch); }
    return t;
  }
  const int m = (int)nodes.size();
  if (seg_tiles(m) >= 2 && m >= 3) {
    constexpr int kArr = 3;
    std::vector<int> arr[kArr], ls;
    pseudo_peripheral(S, nodes, arr[0], ls);  // (leaves S.in = nodes)
    arr[1].assign(arr[0].rbegin(), arr[0].rend());
    arr[2] = nodes;  // ascending: the caller's order
    std::vector<int> pos((size_t)S.g.n, 0), far((size_t)m, 0);
    WindowCut cut;
    int which = -1;
    for (int a = 0; a < kArr; ++a) best_window(S.g, S.in, arr[a], pos, far, cut, which, a);
    if (which >= 0 && cut.cost <= seg_tiles(m)) {
      std::vector<int> A, sep, B;
      if (split_at_window(S, arr[which], cut.lo, cut.hi, A, sep, B)) {
        std::sort(A.begin(), A.end()); std::sort(B.begin(), B.end()); std::sort(sep.begin(), sep.end());
        Tree cand(1);
        const int ca = graft(cand, cut_dissect(S, A, move_up));
        const int cb = graft(cand, cut_dissect(S, B, move_up));
        cand[0].child = {ca, cb};
        rcm(S, sep, cand[0].cams);
        int up = 0;
        if (chain_tiles(cand, 0, false, move_up, up) < seg_tiles(m)) return cand;  // kept only if it shortens the part's chain
      }
    }
  }
  rcm(S, nodes, t[0].cams);
  return t;
}

// ---- dissection to a GIVEN chain (round 14) -------------------------------------------------------------------------------------
// cut_dissect() takes every part's best single cut.  That balances a cut in the tiles of its two sides as they are, not as they
// will be once they are cut themselves: at C3 one half of the orbit came out a tile column longer than the other (a leaf chain
// of four beside one of two), and the root waited for it.  fit_dissect() asks the other way round: can this part be laid out
// with a chain of at most T tile columns?  A part that fits T undivided gets its greedy tree (refit(), below, keeps every
// greedy subtree that is short enough: only parts on the critical path are cut differently, or once more).  Otherwise the part
// is laid out breadth-first from a pseudo-peripheral camera and smoothed, and for every separator size in tiles ts < T, the window that leaves
// the smaller larger side is tried (for sides of one kind, the one with fewer cameras fits if any does), and both sides must
// fit T - ts.  The hand-over of flatten() is counted where a size is turned into tiles (a segment a camera or two over a tile
// boundary is a tile shorter), and every tree that is put together is checked with chain_tiles(), which knows what the
// children hand up.  Depth first, the first tree that fits wins; `budget` counts down the cameras of the parts laid out.
inline int handed_tiles(int cams, bool is_root, int move_up) {  // tiles of a segment after the hand-over, as in flatten()
  if (!is_root) {
    const int whole = (6 * cams) / kTileCols * kTileCols / 6, over = cams - whole;
    if (over > 0 && over <= move_up && whole > 0 && (6 * cams) % kTileCols != 0) cams = whole;
  }
  return seg_tiles(cams);
}

// A breadth-first order lists the cameras of one level in the order of the caller's numbering, and a window is as wide as the
// worst of them.  Here every camera moves to the mean position of itself and its neighbours, twice: inside a level the cameras
// that see further back come first, whatever they are called (pos: scratch of g.n entries).
void smoothed(const CamGraph& g, const Mask& in, const std::vector<int>& from, std::vector<int>& pos, std::vector<int>& out) {
  const int m = (int)from.size();
  out = from;
  std::vector<std::pair<double, int>> key((size_t)m);
  for (int sweep = 0; sweep < 2; ++sweep) {
    for (int q = 0; q < m; ++q) pos[(size_t)out[(size_t)q]] = q;
    for (int q = 0; q < m; ++q) {
      long sum = q, cnt = 1;
      const uint64_t* r = g.row(out[(size_t)q]);
      for (int w = 0; w < g.words; ++w) {
        uint64_t b = r[w] & in[(size_t)w];
        while (b) { sum += pos[(size_t)(w * 64 + __builtin_ctzll(b))]; ++cnt; b &= b - 1; }
      }
      key[(size_t)q] = {(double)sum / (double)cnt, q};
    }
    std::sort(key.begin(), key.end());
    std::vector<int> next((size_t)m);
    for (int q = 0; q < m; ++q) next[(size_t)q] = out[(size_t)key[(size_t)q].second];
    out.swap(next);
  }
}

bool fit_dissect(Sub& S, const std::vector<int>& nodes, int T, bool is_root, int move_up, int& budget, Tree& out) {
  const int m = (int)nodes.size();
  if (T <= 0 || (budget -= m) < 0) return false;
  std::vector<std::vector<int>> comps;
  components(S, nodes, comps);
  if (comps.size() > 1) {
    Tree t(1);
    for (const auto& c : comps) {
      Tree sub;
      if (!fit_dissect(S, c, T, false, move_up, budget, sub)) return false;
      const int ch = graft(t, std::move(sub));
      t[0].child.push_back(ch);
    }
    int up = 0;
    if (chain_tiles(t, 0, is_root, move_up, up) > T) return false;
    out = std::move(t);
    return true;
  }
  int up = 0;
  if (handed_tiles(m, is_root, move_up) <= T) {  // fits undivided: the greedy tree, which is no longer than that
    Tree greedy = cut_dissect(S, nodes, move_up);
    if (chain_tiles(greedy, 0, is_root, move_up, up) > T) return false;
    out = std::move(greedy);
    return true;
  }
  if (m < 3) return false;
  constexpr int kArr = 2;  // breadth-first from a pseudo-peripheral camera, smoothed; forwards and backwards
  std::vector<int> arr[kArr], pos((size_t)S.g.n, 0), far[kArr], near[kArr], ls;
  {
    std::vector<int> bfs;
    pseudo_peripheral(S, nodes, bfs, ls);  // (leaves S.in = nodes)
    smoothed(S.g, S.in, bfs, pos, arr[0]);
  }
  arr[1].assign(arr[0].rbegin(), arr[0].rend());
  for (int a = 0; a < kArr; ++a) { far[a].resize((size_t)m); near[a].resize((size_t)m); }
  reach_of(S.g, S.in, arr[0], pos, far[0], &near[0]);
  for (int q = 0; q < m; ++q) { far[1][(size_t)(m - 1 - q)] = m - 1 - near[0][(size_t)q]; near[1][(size_t)(m - 1 - q)] = m - 1 - far[0][(size_t)q]; }
  struct Win { int arr = -1, lo = 0, hi = 0, side = 0, sep = 0, ts = 0; };
  std::vector<Win> wins;
  int ts_min = T;
  for (int a = 0; a < kArr; ++a)
    windows_of(far[a], &near[a], m, [&](int c, int e, int nl, int ns, int nr) {
      const int ts = handed_tiles(ns, is_root, move_up);
      ts_min = std::min(ts_min, ts);
      if (ts < T) wins.push_back(Win{a, c, e, std::max(nl, nr), ns, ts});
    });
  // A side larger than what T - ts tiles can hold is not tried.  What they can hold is reckoned with separators half as wide as
  // the narrowest of THIS part, in tiles, for every cut below (half: a window of an orbit cuts two fronts, the windows of its
  // arcs one).  True of a graph that looks the same everywhere, a guess elsewhere — which may miss a tree there, and keeps a
  // search that cannot succeed from walking the whole part.
  const int ts_below = (ts_min + 1) / 2;
  std::vector<int> holds((size_t)T, 0);  // [t]: cameras a chain of t tiles can hold
  for (int k = 1; k < T; ++k) {
    const auto leaf = [&](int t) { return kTileCols * t / 6 + move_up; };
    holds[(size_t)k] = std::max(leaf(k), k > ts_below ? 2 * holds[(size_t)(k - ts_below)] + leaf(ts_below) : 0);
  }
  std::vector<Win> by_tiles((size_t)T);  // [ts]: the window of ts separator tiles with the smaller larger side
  for (const Win& c : wins) {
    Win& w = by_tiles[(size_t)c.ts];
    if (c.side > holds[(size_t)(T - c.ts)]) continue;
    if (w.arr < 0 || c.side < w.side || (c.side == w.side && c.sep < w.sep)) w = c;
  }
  for (int ts = 1; ts < T; ++ts) {
    const Win& w = by_tiles[(size_t)ts];
    if (w.arr < 0) continue;
    std::vector<int> A, sep, B;
    if (!split_at_window(S, arr[w.arr], w.lo, w.hi, A, sep, B)) continue;
    std::sort(A.begin(), A.end()); std::sort(B.begin(), B.end()); std::sort(sep.begin(), sep.end());
    const int rest = T - handed_tiles((int)sep.size(), is_root, move_up);
    Tree cand(1), left, right;
    if (!fit_dissect(S, A, rest, false, move_up, budget, left) || !fit_dissect(S, B, rest, false, move_up, budget, right)) continue;
    const int ca = graft(cand, std::move(left));
    const int cb = graft(cand, std::move(right));
    cand[0].child = {ca, cb};
    rcm(S, sep, cand[0].cams);
    if (chain_tiles(cand, 0, is_root, move_up, up) <= T) { out = std::move(cand); return true; }
  }
  return false;
}

void subtree_cams(const Tree& t, int node, std::vector<int>& cams) {
  cams.insert(cams.end(), t[(size_t)node].cams.begin(), t[(size_t)node].cams.end());
  for (int c : t[(size_t)node].child) subtree_cams(t, c, cams);
}
Tree subtree(const Tree& t, int node) {
  Tree s(1);
  s[0].cams = t[(size_t)node].cams;
  for (int c : t[(size_t)node].child) { const int ch = graft(s, subtree(t, c)); s[0].child.push_back(ch); }
  return s;
}

// A tree brought to a chain of at most T tile columns with as little of it cut anew as will do: a subtree that is short enough
// stays; one that is not first keeps its separator and shortens what is too long below it, and only if that fails is laid
// out again as a whole by fit_dissect().  On the greedy tree of C3 this re-cuts one eighth of the orbit.
bool refit(Sub& S, const Tree& t, int node, int T, bool is_root, int move_up, int& budget, Tree& out) {
  int up = 0;
  if (chain_tiles(t, node, is_root, move_up, up) <= T) { out = subtree(t, node); return true; }
  if (T <= 0 || budget < 0) return false;
  const Seg& seg = t[(size_t)node];
  const int rest = T - (seg.cams.empty() ? 0 : handed_tiles((int)seg.cams.size(), is_root, move_up));
  if (!seg.child.empty() && rest > 0) {
    Tree cand(1);
    cand[0].cams = seg.cams;
    bool ok = true;
    for (int c : seg.child) {
      Tree sub;
      if (!(ok = refit(S, t, c, rest, false, move_up, budget, sub))) break;
      const int ch = graft(cand, std::move(sub));
      cand[0].child.push_back(ch);
    }
    if (ok && chain_tiles(cand, 0, is_root, move_up, up) <= T) { out = std::move(cand); return true; }
  }
  std::vector<int> nodes;
  subtree_cams(t, node, nodes);
  std::sort(nodes.begin(), nodes.end());
  return fit_dissect(S, nodes, T, is_root, move_up, budget, out);
}

}  // namespace

void order_cameras(const CamGraph& g, int depth, int move_up, std::vector<int32_t>& slot_of_nat, std::vector<int32_t>& col_of_slot, int& n_cols) {
  slot_of_nat.assign((size_t)g.n, -1);
  col_of_slot.assign((size_t)g.n, 0);
  if (depth < 0 || g.n == 0) {
    for (int i = 0; i < g.n; ++i) { slot_of_nat[(size_t)i] = i; col_of_slot[(size_t)i] = 6 * i; }
    n_cols = 6 * g.n;
    return;
  }
  Sub S(g);
  std::vector<Seg> tree;
  std::vector<int> all((size_t)g.n);
  for (int i = 0; i < g.n; ++i) all[(size_t)i] = i;
  dissect(S, tree, all, depth);
  slots_from_tree(tree, g.n, move_up, slot_of_nat, col_of_slot, n_cols);
}

void tile_pattern(const CamGraph& g, const std::vector<int32_t>& slot_of_nat, const std::vector<int32_t>& col_of_slot, int n_cols,
                  std::vector<uint8_t>& pat, int& nt) {
  nt = (n_cols + 31) / 32;
  pat.assign((size_t)nt * (size_t)nt, 0);
  auto mark = [&](int sa, int sb) {
    const int ca = col_of_slot[(size_t)sa], cb = col_of_slot[(size_t)sb];
    const int a0 = ca / 32, a1 = (ca + 5) / 32, b0 = cb / 32, b1 = (cb + 5) / 32;
    for (int a = a0; a <= a1; ++a)
      for (int b = b0; b <= b1; ++b) { if (a > b) pat[(size_t)a * nt + b] = 1; else if (b > a) pat[(size_t)b * nt + a] = 1; }
  };
  for (int i = 0; i < g.n; ++i) {
    const int si = slot_of_nat[(size_t)i];
    mark(si, si);
    const uint64_t* r = g.row(i);
    for (int w = 0; w < g.words; ++w) {
      uint64_t m = r[w];
      while (m) {
        const int j = w * 64 + __builtin_ctzll(m);
        m &= m - 1;
        if (j > i && j < g.n) mark(si, slot_of_nat[(size_t)j]);
      }
    }
  }
}

void level_heads(CholPlan& P) {
  P.heads.assign(P.items.size(), LevelHead{});
  for (size_t q = 0; q < P.items.size(); ++q) {
    const CholItem& it = P.items[q];
    LevelHead& H = P.heads[q];
    H.type = it.type; H.ti = it.ti; H.tk = it.tk; H.nsrc = it.nsrc;
    if (it.type == kItemRole) {
      for (int r = 0; r < std::min<int>(it.nsrc, kHeadRows); ++r) H.row[r] = P.rows[(size_t)it.aux + r];
      H.over = it.aux + kHeadRows;
    } else {
      for (int r = 0; r < std::min<int>(it.nsrc, kInlineSrc); ++r) H.src[r] = P.srcs[(size_t)it.src + r];
      H.over = it.src + kInlineSrc;
    }
  }
}

void plan_from_pattern(const std::vector<uint8_t>& pat, int nt, bool use_pinv, int inv_rows, CholPlan& P, bool tables) {
  P.nt = nt; P.use_pinv = use_pinv;
  P.struct_start.assign((size_t)nt + 1, 0); P.struct_rows.clear();
  P.parent.assign((size_t)nt, -1); P.level.assign((size_t)nt, 0);
  P.items.clear(); P.launch_start.clear(); P.srcs.clear(); P.rows.clear(); P.heads.clear(); P.asm_tiles.clear();
  P.back_cols.clear(); P.back_start.clear();
  P.products = 0; P.roles = 0; P.nlevels = 0;
  if (nt <= 0) { P.launch_start.push_back(0); P.back_start.push_back(0); return; }
  const int W = (nt + 1 + 63) / 64;
  // symbolic factorisation: struct(j) = pattern of column j below the diagonal, plus struct(c) \ {j} of the children c
  std::vector<uint64_t> st((size_t)nt * (size_t)W, 0);
  std::vector<std::vector<int>> children((size_t)nt);
  auto bit = [&](int j, int i) -> bool { return (st[(size_t)j * W + (i >> 6)] >> (i & 63)) & 1; };
  for (int j = 0; j < nt; ++j) {
    uint64_t* s = st.data() + (size_t)j * W;
    for (int i = j + 1; i < nt; ++i) if (pat[(size_t)i * nt + j]) s[i >> 6] |= 1ull << (i & 63);
    s[nt >> 6] |= 1ull << (nt & 63);  // the right-hand-side row
    for (int c : children[(size_t)j]) {
      const uint64_t* sc = st.data() + (size_t)c * W;
      for (int w = 0; w < W; ++w) s[w] |= sc[w];
    }
    for (int i = 0; i <= j; ++i) s[i >> 6] &= ~(1ull << (i & 63));
    int par = -1;
    for (int i = j + 1; i < nt; ++i) if (bit(j, i)) { par = i; break; }
    P.parent[(size_t)j] = par;
    if (par >= 0) children[(size_t)par].push_back(j);
    int lv = 0;
    for (int c : children[(size_t)j]) lv = std::max(lv, P.level[(size_t)c] + 1);
    P.level[(size_t)j] = lv;
    P.nlevels = std::max(P.nlevels, lv + 1);
  }
  for (int j = 0; j < nt; ++j) {
    for (int i = j + 1; i <= nt; ++i) if (bit(j, i)) P.struct_rows.push_back(i);
    P.struct_start[(size_t)j + 1] = (int32_t)P.struct_rows.size();
  }
  // a reduced system without exploitable structure would need a table of ~nt^3/6 tile products: leave the item tables
  // empty (nlevels = 0) and let the caller fall back to the dense outer-panel path
  {
    double prod = 0.0;
    for (int j = 0; j < nt; ++j) { const double sj = (double)(P.struct_start[(size_t)j + 1] - P.struct_start[(size_t)j]); prod += 0.5 * sj * (sj + 1.0); }
    if (prod > kMaxPlanProducts) {
      P.products = (int64_t)prod; P.nlevels = 0; P.est_us = 1e30;
      P.launch_start.assign(1, 0); P.back_start.assign(1, 0);
      return;
    }
    if (!tables) {  // candidate comparison: every column's struct(j) (struct(j) + 1) / 2 tile products, roles over the subtree sizes
      P.products = (int64_t)prod;
      if (use_pinv) {
        std::vector<int64_t> sub((size_t)nt, 1);
        for (int j = 0; j < nt; ++j) {
          if (P.parent[(size_t)j] >= 0) sub[(size_t)P.parent[(size_t)j]] += sub[(size_t)j];
          const int64_t nrr = P.struct_start[(size_t)j + 1] - P.struct_start[(size_t)j] - 1;
          P.roles += sub[(size_t)j] * ((nrr + inv_rows - 1) / std::max(inv_rows, 1));
        }
      }
      P.est_us = 9.5 * P.nlevels + 0.02 * (double)P.products + 0.004 * (double)P.roles + (use_pinv ? 10.0 : 6.5 * P.nlevels);
      return;
    }
  }
  auto rows_of = [&](int j) { return std::make_pair(P.struct_rows.data() + P.struct_start[(size_t)j], P.struct_rows.data() + P.struct_start[(size_t)j + 1]); };
  auto lt = [](int64_t ti, int64_t tj) { return (int32_t)(ti * (ti + 1) / 2 + tj); };
  for (int j = 0; j < nt; ++j) {
    P.asm_tiles.push_back(lt(j, j));
    auto r = rows_of(j);
    for (const int32_t* p = r.first; p != r.second; ++p) P.asm_tiles.push_back(lt(*p, j));
  }
  std::sort(P.asm_tiles.begin(), P.asm_tiles.end());
  // subtree lists (inverse roles): the descendants of j, j included
  std::vector<std::vector<int>> subtree;
  if (use_pinv) {
    subtree.resize((size_t)nt);
    for (int j = 0; j < nt; ++j) {
      for (int c : children[(size_t)j]) subtree[(size_t)j].insert(subtree[(size_t)j].end(), subtree[(size_t)c].begin(), subtree[(size_t)c].end());
      subtree[(size_t)j].push_back(j);
      std::sort(subtree[(size_t)j].begin(), subtree[(size_t)j].end());
    }
  }
  std::vector<std::vector<int>> by_level((size_t)P.nlevels);
  for (int j = 0; j < nt; ++j) by_level[(size_t)P.level[(size_t)j]].push_back(j);
  // launch l: the panels of the columns of level l; trailing updates and inverse roles from the columns of level l-1
  for (int l = 0; l < P.nlevels; ++l) {
    P.launch_start.push_back((int32_t)P.items.size());
    for (int c : by_level[(size_t)l]) {
      // children whose level is l-1 reach column c through the panel items; deeper children went through trailing items
      std::vector<int> kids;
      for (int k : children[(size_t)c]) if (P.level[(size_t)k] == l - 1) kids.push_back(k);
      auto r = rows_of(c);
      for (int q = -1; q < (int)(r.second - r.first); ++q) {
        const int ti = q < 0 ? c : r.first[q];
        CholItem it{kItemPanel, (uint16_t)ti, (uint16_t)c, (uint16_t)kids.size(), (uint32_t)P.srcs.size(), 0};
        for (int k : kids) P.srcs.push_back(k | ((ti != c && bit(k, ti)) ? kSrcX : 0));
        P.items.push_back(it);
      }
    }
    if (l == 0) continue;
    if (use_pinv) {
      for (int j : by_level[(size_t)l - 1]) {
        auto r = rows_of(j);
        const int nrr = (int)(r.second - r.first) - 1;  // without the right-hand-side row
        for (int g0 = 0; g0 < nrr; g0 += inv_rows) {
          const int nr = std::min(inv_rows, nrr - g0);
          const uint32_t off = (uint32_t)P.rows.size();
          for (int q = 0; q < nr; ++q) P.rows.push_back(r.first[g0 + q]);
          for (int k : subtree[(size_t)j]) { P.items.push_back(CholItem{kItemRole, (uint16_t)j, (uint16_t)k, (uint16_t)nr, 0, off}); ++P.roles; }
        }
      }
    }
    std::map<std::pair<int, int>, std::vector<int>> trail;  // (tk, ti) -> source columns
    for (int k : by_level[(size_t)l - 1]) {
      auto r = rows_of(k);
      const int par = P.parent[(size_t)k];
      for (const int32_t* pk = r.first; pk != r.second; ++pk) {
        const int tk = *pk;
        if (tk >= nt) continue;
        if (tk == par && P.level[(size_t)par] == l) continue;  // the panel items of column par take this source
        for (const int32_t* pi = pk; pi != r.second; ++pi) trail[{tk, *pi}].push_back(k);
      }
    }
    for (auto& e : trail) {
      CholItem it{kItemTrail, (uint16_t)e.first.second, (uint16_t)e.first.first, (uint16_t)e.second.size(), (uint32_t)P.srcs.size(), 0};
      for (int k : e.second) P.srcs.push_back(k);
      P.items.push_back(it);
      P.products += (int64_t)e.second.size();
    }
  }
  P.launch_start.push_back((int32_t)P.items.size());
  for (const CholItem& it : P.items) if (it.type == kItemPanel) P.products += it.nsrc;
  for (int l = P.nlevels - 1; l >= 0; --l) {
    P.back_start.push_back((int32_t)P.back_cols.size());
    for (int j : by_level[(size_t)l]) P.back_cols.push_back(j);
  }
  P.back_start.push_back((int32_t)P.back_cols.size());
  level_heads(P);
  // launch-cost model (measured on MI355X: a dependent launch ~9.5 us whatever it holds up to a few hundred workgroups)
  P.est_us = 9.5 * P.nlevels + 0.02 * (double)P.products + 0.004 * (double)P.roles + (use_pinv ? 10.0 : 6.5 * P.nlevels);
}

void plan_auto(const CamGraph& g, int forced_depth, bool forced, bool cuts, int pinv_max_tiles, int inv_rows, CholPlan& best, PlanParallelFor pfor) {
  int dmax = -1;
  for (int s = g.n; s >= kMinLeaf / 2; s /= 2) ++dmax;  // candidate depths down to parts of ~kMinLeaf / 2 cameras (dissect() itself
  dmax = std::min(dmax, 6);                             // stops at kMinLeaf); the cost model decides (C3: depth 3, 14 levels)
  // the candidate orders are independent: evaluated side by side on host threads when the graph is large (C4: 6 ms one after
  // the other), the cheapest by the launch-cost model wins, ties go to the first in this list (what the sequential loop chose)
  // cut: an order from the dissection by window separators (below).  Its tree is built and rated by tile arithmetic beside the
  // legacy candidates (`chain`, O(cameras)); `rated`: it has its symbolic factorisation too
  // fit: a cut candidate of the second pass, dissected to a given chain (fit_dissect) from what its first-pass twin reached
  struct Cand { int depth, move_up; CholPlan P; std::vector<uint8_t> pat; bool cut = false, rated = false; int chain = 0; bool fit = false; Tree tree; };
  std::vector<Cand> cands;
  cands.reserve(32);  // (never grows beyond: the passes hold pointers into it)
  for (int d = -1; d <= (forced ? -1 : dmax); ++d) {
    const int depth = forced ? forced_depth : d;
    for (int move_up : {0, 2, 4}) {
      if (depth < 1 && move_up > 0) break;  // nothing to move without separators
      cands.push_back(Cand{depth, move_up, CholPlan(), {}});
    }
  }
  const size_t n_legacy = cands.size();
  if (cuts && !forced && g.n >= kMinCutCams)
    for (int move_up : {0, 2, 4}) { cands.push_back(Cand{0, move_up, CholPlan(), {}}); cands.back().cut = true; }
  const size_t n_greedy = cands.size();
  auto evaluate = [&](Cand& c) {
    CholPlan& P = c.P;
    if (c.cut && !c.rated) {  // first pass: the tree, its chain in tiles and the order it gives
      Sub S(g);
      std::vector<int> all((size_t)g.n);
      for (int i = 0; i < g.n; ++i) all[(size_t)i] = i;
      c.tree = cut_dissect(S, all, c.move_up);
      int up = 0;
      c.depth = tree_depth(c.tree, 0);
      c.chain = chain_tiles(c.tree, 0, true, c.move_up, up);
      slots_from_tree(c.tree, g.n, c.move_up, P.slot_of_nat, P.col_of_slot, P.n);
      return;
    }
    if (c.fit) {  // second pass: the greedy tree (c.tree) brought to the chain c.chain, then its symbolic factorisation
      Sub S(g);
      Tree found;
      int up = 0, budget = kFitWork * g.n;
      if (!refit(S, c.tree, 0, c.chain, true, c.move_up, budget, found)) { c.rated = false; return; }
      c.tree.swap(found);
      c.depth = tree_depth(c.tree, 0);
      c.chain = chain_tiles(c.tree, 0, true, c.move_up, up);
      slots_from_tree(c.tree, g.n, c.move_up, P.slot_of_nat, P.col_of_slot, P.n);
    }
    P.ncv = g.n; P.nd_depth = c.depth;
    P.nslots = g.n;
    if (!c.cut) order_cameras(g, c.depth, c.move_up, P.slot_of_nat, P.col_of_slot, P.n);
    int nt = 0;
    tile_pattern(g, P.slot_of_nat, P.col_of_slot, P.n, c.pat, nt);
    plan_from_pattern(c.pat, nt, nt <= pinv_max_tiles, inv_rows, P, /*tables=*/false);
  };
  auto evaluate_all = [&](const std::vector<Cand*>& todo) {
    const size_t cnt = todo.size();
    if (pfor && g.n >= 64 && cnt > 1) {  // the caller's persistent workers (C3: 0.5 -> 0.15 ms; C4: 6.3 -> 1.9 ms)
      struct Ctx { decltype(evaluate)* ev; Cand* const* c; } ctx{&evaluate, todo.data()};
      pfor((int)cnt, [](void* p, int i) { Ctx* x = static_cast<Ctx*>(p); (*x->ev)(*x->c[i]); }, &ctx);
    } else if (g.n >= 256 && cnt > 1) {
      std::vector<std::thread> th;
      for (size_t i = 1; i < cnt; ++i) th.emplace_back([&, i] { evaluate(*todo[i]); });
      evaluate(*todo[0]);
      for (auto& x : th) x.join();
    } else {
      for (Cand* c : todo) evaluate(*c);
    }
  };
  std::vector<Cand*> todo;
  for (Cand& c : cands) todo.push_back(&c);
  evaluate_all(todo);
  size_t bi = 0;
  for (size_t i = 1; i < n_legacy; ++i)
    if (cands[i].P.est_us < cands[bi].P.est_us - 1e-9) bi = i;
  const size_t legacy = bi;
  size_t greedy = legacy;  // the choice without the fitted trees (what round 12 took): what stands if a fitted plan is refused below
  // The second family: dissection by minimal window separators.  Only the best few trees by their arithmetic (an upper bound
  // of the levels, met on every graph tried) get a symbolic factorisation, and only where the arithmetic promises a gain.
  // Not taken on a short chain (fewer than kMinCutLevels levels: at most a launch or two to gain, against more padding
  // columns), which also keeps small systems on the plans the kernels' tests are built around.
  if (cands.size() > n_legacy && cands[legacy].P.nlevels >= kMinCutLevels) {
    constexpr size_t kMaxCutCands = 2;
    const int want = cands[legacy].P.nlevels - kMinCutGain;  // a chain worth a symbolic factorisation
    todo.clear();
    for (size_t i = n_legacy; i < n_greedy; ++i) {
      Cand& c = cands[i];
      bool known = c.depth < 1 || c.chain > want;  // nothing was cut, or too little to gain
      for (const Cand* o : todo) known = known || (o->P.slot_of_nat == c.P.slot_of_nat && o->P.col_of_slot == c.P.col_of_slot);
      if (!known) todo.push_back(&c);
    }
    std::stable_sort(todo.begin(), todo.end(), [](const Cand* a, const Cand* b) { return a->chain < b->chain; });
    if (todo.size() > kMaxCutCands) todo.resize(kMaxCutCands);
    // ... and beside them one fitted tree per hand-over limit: a chain at least one tile column below the greedy tree's, and
    // short enough to be taken
    for (size_t i = n_legacy; i < n_greedy; ++i) {
      if (cands[i].depth < 1) continue;
      cands.push_back(Cand{0, cands[i].move_up, CholPlan(), {}});
      cands.back().cut = cands.back().fit = true;
      cands.back().chain = std::min(cands[i].chain - 1, want);
      cands.back().tree = cands[i].tree;
    }
    for (size_t i = n_greedy; i < cands.size(); ++i) todo.push_back(&cands[i]);
    for (Cand* c : todo) c->rated = true;
    if (!todo.empty()) evaluate_all(todo);
    // A cut-search order replaces the legacy choice only with fewer levels (by kMinCutGain), and only if it keeps the inverse
    // accumulators where the legacy plan has them; among several, the fewest levels, then the cost model.
    const CholPlan& L = cands[legacy].P;
    for (size_t i = n_legacy; i < cands.size(); ++i) {
      if (i == n_greedy) greedy = bi;
      const CholPlan& C = cands[i].P;
      if (!cands[i].rated || C.nlevels <= 0 || C.nlevels + kMinCutGain > L.nlevels || (L.nt <= pinv_max_tiles && C.nt > pinv_max_tiles)) continue;
      if (bi == legacy || C.nlevels < cands[bi].P.nlevels || (C.nlevels == cands[bi].P.nlevels && C.est_us < cands[bi].P.est_us - 1e-9)) bi = i;
    }
    if (cands.size() == n_greedy) greedy = bi;
  }
  // ... and only if its items stay in the unrolled forms of k_chol_level (a panel with up to kFastPanelSrc sources, a trailing
  // tile with up to kFastTrailSrc): a level of the slower list loops can cost what a level less saves.  A fitted plan that does
  // not gives way to the greedy tree's, that one to the legacy plan, which, as on any tie or loss above, stands as it was, table
  // for table.
  std::vector<uint8_t> best_pat;
  const size_t picks[3] = {bi, greedy, legacy};
  for (int k = 0; k < 3; ++k) {
    const size_t pick = picks[k];
    if (k > 0 && pick == picks[k - 1]) continue;  // (refused a moment ago)
    best = std::move(cands[pick].P);
    best_pat = std::move(cands[pick].pat);
    plan_from_pattern(best_pat, best.nt, best.nt <= pinv_max_tiles, inv_rows, best, /*tables=*/true);
    if (pick == legacy) break;
    int psrc = 0, tsrc = 0;
    for (const CholItem& it : best.items) {
      if (it.type == kItemPanel) psrc = std::max<int>(psrc, it.nsrc);
      if (it.type == kItemTrail) tsrc = std::max<int>(tsrc, it.nsrc);
    }
    if (psrc <= kFastPanelSrc && tsrc <= kFastTrailSrc) break;
  }
  best.nat_of_slot.assign((size_t)best.nslots, -1);
  for (int i = 0; i < g.n; ++i) best.nat_of_slot[(size_t)best.slot_of_nat[(size_t)i]] = i;
  best.slot_of_col.assign((size_t)best.n, -1);
  for (int sl = 0; sl < best.nslots; ++sl)
    for (int a = 0; a < 6; ++a) best.slot_of_col[(size_t)best.col_of_slot[(size_t)sl] + a] = sl * 8 + a;
}

}  // namespace mpsfm

// ---- test hook: the plan of a camera graph, without a device (tests/test_chol_plan_cpu.py interprets the item tables with
// NumPy and compares with a dense Cholesky) ------------------------------------------------------------------------------
extern "C" {

struct mpsfm_plan_handle { mpsfm::CholPlan P; };

// adj: n x n bytes (symmetric, nonzero = the cameras share a landmark).  depth -2: choose among the level-structure dissections;
// -3: what a handle does by default (the window-separator orders compete too); >= -1: that order.
mpsfm_plan_handle* mpsfm_debug_plan_create(const uint8_t* adj, int32_t n, int32_t depth, int32_t pinv_max_tiles, int32_t inv_rows) {
  if (!adj || n < 0 || depth < -3) return nullptr;
  mpsfm::CamGraph g;
  g.init(n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) if (i != j && adj[(size_t)i * n + j]) g.set(i, j);
  auto* h = new mpsfm_plan_handle();
  // (-3 on the host threads a handle plans with, MPSFM_HOST_THREADS: the plan must not depend on how many there are)
  mpsfm::plan_auto(g, depth, depth >= -1, /*cuts=*/depth == -3, pinv_max_tiles, inv_rows, h->P,
                   depth != -3 ? nullptr : [](int n, void (*fn)(void*, int), void* ctx) { mpsfm::run_parts(n, [&](int t, int) { fn(ctx, t); }); });
  return h;
}
void mpsfm_debug_plan_destroy(mpsfm_plan_handle* h) { delete h; }
// what: 0 header {ncv, nslots, n, nt, nlevels, nd_depth, use_pinv, n_items, products, roles}; 1 slot_of_nat; 2 struct_start; 3 struct_rows;
// 4 parent; 5 level; 6 items (4 int32 each: type | ti << 16, tk | nsrc << 16, src, aux); 7 launch_start; 8 srcs; 9 rows; 10 asm_tiles;
// 11 back_cols; 12 back_start; 13 col_of_slot; 14 heads (the launch records as they go to the device, 16 int32 each: type | ti << 16,
// tk | nsrc << 16, kInlineSrc sources, kHeadRows rows, overflow offset, 0).  Returns the length; copies min(length, cap) entries.
int64_t mpsfm_debug_plan_get(const mpsfm_plan_handle* h, int32_t what, int32_t* out, int64_t cap) {
  if (!h) return -1;
  const mpsfm::CholPlan& P = h->P;
  std::vector<int32_t> tmp;
  const std::vector<int32_t>* v = &tmp;
  switch (what) {
    case 0: tmp = {P.ncv, P.nslots, P.n, P.nt, P.nlevels, P.nd_depth, P.use_pinv ? 1 : 0, (int32_t)P.items.size(), (int32_t)P.products, (int32_t)P.roles}; break;
    case 1: v = &P.slot_of_nat; break;
    case 2: v = &P.struct_start; break;
    case 3: v = &P.struct_rows; break;
    case 4: v = &P.parent; break;
    case 5: v = &P.level; break;
    case 6:
      for (const mpsfm::CholItem& it : P.items) {
        tmp.push_back((int32_t)(it.type | ((uint32_t)it.ti << 16))); tmp.push_back((int32_t)(it.tk | ((uint32_t)it.nsrc << 16)));
        tmp.push_back((int32_t)it.src); tmp.push_back((int32_t)it.aux);
      }
      break;
    case 7: v = &P.launch_start; break;
    case 8: v = &P.srcs; break;
    case 9: v = &P.rows; break;
    case 10: v = &P.asm_tiles; break;
    case 11: v = &P.back_cols; break;
    case 12: v = &P.back_start; break;
    case 13: v = &P.col_of_slot; break;
    case 14:
      static_assert(sizeof(mpsfm::LevelHead) == 16 * sizeof(int32_t), "heads are handed out as int32");
      tmp.resize(P.heads.size() * 16);
      if (!P.heads.empty()) std::memcpy(tmp.data(), P.heads.data(), sizeof(int32_t) * tmp.size());
      break;
    default: return -1;
  }
  if (out) std::memcpy(out, v->data(), sizeof(int32_t) * (size_t)std::min<int64_t>(cap, (int64_t)v->size()));
  return (int64_t)v->size();
}

}  // extern "C"
