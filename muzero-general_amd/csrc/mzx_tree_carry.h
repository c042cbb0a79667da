// mzx_tree_carry.h -- searches that continue from searched trees (MCTS.run(..., override_root_with=node) on a node that
// already carries visits and expanded descendants, /root/reference/self_play.py:260-361).
//
//   tree_advance_kernel   tree i, action a_i -> a compact tree whose root is root.children[a_i] (a_i = -1: the old root
//                         itself), copied from a source arena into a destination arena (no lane reads a node another lane
//                         has already overwritten): membership, renumbering, slot records, hidden states, root meta.
//   ContinueRootOp        root preparation of a continued search: Dirichlet noise mixed into the priors the root's
//                         children already have, meta words and MinMaxStats reset; no initial_inference.
//   pack_loaded_tree      host-side import of a tree built elsewhere (reference Node graphs flattened in canonical order).
//
// Renumbering (the contract of the continued searches): the kept nodes stay in creation order -- increasing old
// canonical index, the new root at 0 -- so the leaf expanded by continued simulation k gets index n_carried + k, exactly
// the order the reference's Node graph was grown in.  A node is kept if it is the chosen child or its parent is kept;
// parents precede their children in canonical order, so one pass over the nodes in increasing order decides membership.
#pragma once
#include "../../include/mzx.h"
#include "mzx_launch.h"
#include "mzx_ops.h"

namespace mzx {

enum { TF_BAD_CARRY = 4 };   // TM_FLAGS: the chosen child was not an expanded node of the tree (the old root was kept)

struct TreeAdvanceArgs {
  SearchParams p;
  TreeLayout L;
  const char* src_trees;       // [B][L.tree_bytes]
  char* dst_trees;
  const float* src_hidden;     // [B][N][Hf]
  float* dst_hidden;
  int32_t* scratch;            // [B][2 N + 2]: old -> new index (map, first N), new -> old (inv, next N)
  const int32_t* actions;      // [B] chosen root action, -1 = the old root
  int32_t* carry;              // [B][2]: nodes carried, to_play of the new root
};

// ---- per-lane pieces shared by the wavefront kernel and the serial driver of tests/hostcheck

// Old canonical index of the new root (0 for a = -1); *bad when `a` names no expanded child of the root.
MZX_HD inline int carry_root(const TreeRef& src, int nn, int a, bool* bad) {
  *bad = false;
  if (a < 0) return 0;
  const int nr = src.meta(TM_ROOT_N);
  for (int s = 0; s < nr; ++s) {
    if (src.root_action(s) == a) {
      const int c = src.child(0, s);
      if (c > 0 && c < nn) return c;
      break;
    }
  }
  *bad = true;
  return 0;
}

// Membership of node n of the chunk starting at `base`, before the in-chunk fix-up: the chosen node, or a node whose
// parent lies in an earlier chunk and was kept.
MZX_HD inline bool carry_seed(const TreeRef& src, const int32_t* map, int n, int nn, int c, int base) {
  if (n >= nn || n < c) return false;
  if (n == c) return true;
  const int par = src.parent(n);
  return par >= c && par < base && map[par] >= 0;
}

// In-chunk fix-up step: a node whose parent lies in the same chunk is kept once its parent is (`mask`: bit l = node
// base + l kept so far).  Repeated until no bit changes; converges in at most the depth of the chunk's subtree part.
MZX_HD inline bool carry_fixup(const TreeRef& src, int n, int nn, int c, int base, uint64_t mask, bool kept) {
  if (kept || n >= nn || n <= c) return kept;
  const int par = src.parent(n);
  return par >= base && par < n && ((mask >> (par - base)) & 1);
}

// Node record j of the new tree (old node n = inv[j]).
MZX_HD inline void carry_node(const TreeRef& src, const TreeRef& dst, const int32_t* map, const int32_t* inv, int j) {
  const int n = inv[j];
  dst.visit(j) = src.visit(n);
  dst.value_sum(j) = src.value_sum(n);
  dst.reward(j) = src.reward(n);
  dst.to_play(j) = src.to_play(n);
  dst.parent(j) = j == 0 ? -1 : map[src.parent(n)];
  dst.parent_slot(j) = j == 0 ? -1 : src.parent_slot(n);
}

// Child slot s of new node j: prior, cached (visit, q) of the child, link remapped (children of a kept node are kept).
MZX_HD inline void carry_slot(const TreeRef& src, const TreeRef& dst, const int32_t* map, const int32_t* inv, int nn, int j,
                              int s) {
  const int n = inv[j];
  const int ch = src.child(n, s);
  dst.prior(j, s) = src.prior(n, s);
  dst.slot_q(j, s) = src.slot_q(n, s);
  dst.slot_visit(j, s) = src.slot_visit(n, s);
  dst.child(j, s) = (ch >= 0 && ch < nn) ? map[ch] : -1;
}

// Root meta of the new tree (one lane): node count, root children (a carried non-root node was expanded over the
// whole action space: A children in action order), counters and MinMaxStats cleared.
MZX_HD inline void carry_meta(const TreeRef& src, const TreeRef& dst, const SearchParams& p, int c, int cnt, bool bad,
                              int32_t* carry) {
  for (int k = 0; k < TM_WORDS; ++k) dst.meta(k) = 0;
  dst.meta(TM_N_NODES) = cnt;
  dst.meta(TM_FLAGS) = bad ? TF_BAD_CARRY : 0;
  const int nr = c == 0 ? src.meta(TM_ROOT_N) : p.num_actions;
  dst.meta(TM_ROOT_N) = nr;
  for (int s = 0; s < p.num_actions; ++s) dst.root_action(s) = c == 0 ? src.root_action(s) : s;
  dst.mm_min() = MZX_INF;
  dst.mm_max() = -MZX_INF;
  carry[0] = cnt;
  carry[1] = src.to_play(c);
}

MZX_HD inline TreeRef carry_tree(const char* trees, const TreeLayout& L, int b) {
  TreeRef t;
  t.base = const_cast<char*>(trees) + (int64_t)b * L.tree_bytes;
  t.L = L;
  return t;
}

#ifndef MZX_HOSTCHECK
// One wavefront per tree.  Membership chunk by chunk (64 nodes: a ballot, the in-chunk fix-up, the exclusive popcount
// prefix sum gives the new indices), then the node records, the slot records (lanes over (node, slot) pairs) and the
// hidden states (16-byte accesses when a row is a multiple of four floats).  Every store is a vector store.
__global__ void __launch_bounds__(64) tree_advance_kernel(const TreeAdvanceArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int N = a.p.num_nodes, A = a.p.num_actions;
  const TreeRef src = carry_tree(a.src_trees, a.L, b), dst = carry_tree(a.dst_trees, a.L, b);
  int32_t* map = a.scratch + (int64_t)b * (2 * N + 2);
  int32_t* inv = map + N;
  int nn = src.meta(TM_N_NODES);
  nn = nn < 1 ? 1 : (nn > N ? N : nn);
  bool bad;
  const int c = carry_root(src, nn, a.actions[b], &bad);
  int cnt = 0;
  const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (int base = c & ~63; base < nn; base += 64) {
    const int n = base + lane;
    bool kept = carry_seed(src, map, n, nn, c, base);
    uint64_t mask = __ballot(kept);
    for (;;) {
      kept = carry_fixup(src, n, nn, c, base, mask, kept);
      const uint64_t m2 = __ballot(kept);
      if (m2 == mask) break;
      mask = m2;
    }
    const int j = cnt + __popcll(mask & below);
    if (n < nn) map[n] = kept ? j : -1;
    if (kept) inv[j] = n;
    cnt += __popcll(mask);
    __syncthreads();     // (one wave per workgroup: orders the map / inv stores before the next chunk's loads)
  }
  for (int j = lane; j < cnt; j += 64) carry_node(src, dst, map, inv, j);
  for (int f = lane; f < cnt * A; f += 64) carry_slot(src, dst, map, inv, nn, f / A, f % A);
  const int Hf = a.p.hidden_size;
  const float* sh = a.src_hidden + (int64_t)b * N * Hf;
  float* dh = a.dst_hidden + (int64_t)b * N * Hf;
  if ((Hf & 3) == 0) {
    const int q = Hf >> 2;
    for (int64_t f = lane; f < (int64_t)cnt * q; f += 64) {
      const int j = (int)(f / q), e = (int)(f % q);
      reinterpret_cast<float4*>(dh + (int64_t)j * Hf)[e] = reinterpret_cast<const float4*>(sh + (int64_t)inv[j] * Hf)[e];
    }
  } else {
    for (int64_t f = lane; f < (int64_t)cnt * Hf; f += 64) {
      const int j = (int)(f / Hf), e = (int)(f % Hf);
      dh[(int64_t)j * Hf + e] = sh[(int64_t)inv[j] * Hf + e];
    }
  }
  if (lane == 0) carry_meta(src, dst, a.p, c, cnt, bad, a.carry + 2 * b);
}

inline int tree_advance_launch(const TreeAdvanceArgs& a, stream_t stream) {
  hipLaunchKernelGGL(tree_advance_kernel, dim3((unsigned)a.p.num_trees), dim3(64), 0, stream, a);
  return (int)hipGetLastError();
}
#else
// Serial driver of the same per-lane pieces (tests/hostcheck): the 64 lanes of a chunk one after the other, the
// ballots as explicit bit sets.
inline int tree_advance_launch(const TreeAdvanceArgs& a, stream_t) {
  const int N = a.p.num_nodes, A = a.p.num_actions;
  for (int b = 0; b < a.p.num_trees; ++b) {
    const TreeRef src = carry_tree(a.src_trees, a.L, b), dst = carry_tree(a.dst_trees, a.L, b);
    int32_t* map = a.scratch + (int64_t)b * (2 * N + 2);
    int32_t* inv = map + N;
    int nn = src.meta(TM_N_NODES);
    nn = nn < 1 ? 1 : (nn > N ? N : nn);
    bool bad;
    const int c = carry_root(src, nn, a.actions[b], &bad);
    int cnt = 0;
    for (int base = c & ~63; base < nn; base += 64) {
      bool kept[64];
      uint64_t mask = 0;
      for (int l = 0; l < 64; ++l) {
        kept[l] = carry_seed(src, map, base + l, nn, c, base);
        mask |= uint64_t(kept[l]) << l;
      }
      for (;;) {
        uint64_t m2 = 0;
        for (int l = 0; l < 64; ++l) {
          kept[l] = carry_fixup(src, base + l, nn, c, base, mask, kept[l]);
          m2 |= uint64_t(kept[l]) << l;
        }
        if (m2 == mask) break;
        mask = m2;
      }
      for (int l = 0; l < 64; ++l) {
        const int n = base + l;
        const int j = cnt + __builtin_popcountll(mask & ((l == 0) ? 0ull : (~0ull >> (64 - l))));
        if (n < nn) map[n] = kept[l] ? j : -1;
        if (kept[l]) inv[j] = n;
      }
      cnt += __builtin_popcountll(mask);
    }
    for (int j = 0; j < cnt; ++j) carry_node(src, dst, map, inv, j);
    for (int f = 0; f < cnt * A; ++f) carry_slot(src, dst, map, inv, nn, f / A, f % A);
    const int Hf = a.p.hidden_size;
    for (int j = 0; j < cnt; ++j)
      memcpy(a.dst_hidden + ((int64_t)b * N + j) * Hf, a.src_hidden + ((int64_t)b * N + inv[j]) * Hf, sizeof(float) * Hf);
    carry_meta(src, dst, a.p, c, cnt, bad, a.carry + 2 * b);
  }
  return 0;
}
#endif

// Root of a continued search (self_play.py:275-314 with override_root_with = a searched node): the root keeps its
// visits, value sum, reward and children; add_exploration_noise (:467-476) mixes noise[s] into the prior the child in
// slot s already has; MinMaxStats starts empty (:306); root_predicted_value is None (:277), NaN here.
struct ContinueRootOp {
  TreeArena arena;
  SearchParams p;
  const double* noise;           // [B][A] slot order, nullable
  double* root_predicted_value;  // [B] out, nullable
  MZX_HD size_t size() const { return (size_t)p.num_trees; }
  MZX_HD void operator()(size_t i) const {
    const int b = (int)i;
    const TreeRef t = arena.tree(b);
    const int32_t keep[3] = {t.meta(TM_N_NODES), t.meta(TM_ROOT_N), t.meta(TM_FLAGS) & TF_BAD_CARRY};
    for (int k = 0; k < TM_WORDS; ++k) t.meta(k) = 0;
    t.meta(TM_N_NODES) = keep[0];
    t.meta(TM_ROOT_N) = keep[1];
    t.meta(TM_FLAGS) = keep[2];
    t.mm_min() = MZX_INF;
    t.mm_max() = -MZX_INF;
    if (noise) {
      const double* nz = noise + (int64_t)b * p.num_actions;
      for (int s = 0; s < keep[1]; ++s) t.prior(0, s) = root_noisy_prior(t.prior(0, s), nz, s, p.exploration_fraction);
    }
    if (root_predicted_value) root_predicted_value[b] = __builtin_nan("");
  }
};

// Host image of tree b from canonical-order host arrays (mzx_search_load): node records, slot records with the cached
// (visit, q) of each expanded child computed with ucb_score's own expression (self_play.py:396-401), root actions.
// `M` = node slots per tree in the host arrays.  Returns 0, or -1 when the tree is inconsistent.
inline int pack_loaded_tree(const TreeRef& t, const SearchParams& p, const mzx_tree_load& h, int b) {
  const int A = p.num_actions, M = h.max_nodes;
  const int nn = h.h_n_nodes[b];
  const int64_t o = (int64_t)b * M;
  for (int k = 0; k < TM_WORDS; ++k) t.meta(k) = 0;
  t.meta(TM_N_NODES) = nn;
  int nr = 0;
  while (nr < A && h.h_root_actions[(int64_t)b * A + nr] >= 0) ++nr;
  if (nr == 0) return -1;
  t.meta(TM_ROOT_N) = nr;
  for (int s = 0; s < A; ++s) t.root_action(s) = s < nr ? h.h_root_actions[(int64_t)b * A + s] : -1;
  t.mm_min() = MZX_INF;
  t.mm_max() = -MZX_INF;
  for (int n = 0; n < nn; ++n) {
    const int vc = h.h_visit[o + n];
    if (vc < 0 || vc + p.num_sims >= p.num_nodes) return -1;     // the pb_c / sqrt tables cover visit counts < N
    t.visit(n) = vc;
    t.value_sum(n) = h.h_value_sum[o + n];
    t.reward(n) = h.h_reward[o + n];
    t.to_play(n) = h.h_to_play[o + n];
    const int par = h.h_parent[o + n];
    if ((n == 0) != (par < 0) || par >= n) return -1;      // parents precede their children
    t.parent(n) = par;
    t.parent_slot(n) = -1;
  }
  for (int n = 0; n < nn; ++n) {
    const int nc = n == 0 ? nr : A;
    for (int s = 0; s < A; ++s) {
      const int ch = s < nc ? h.h_child[(o + n) * A + s] : -1;
      if (ch >= nn || (ch >= 0 && (ch <= n || h.h_parent[o + ch] != n))) return -1;
      t.prior(n, s) = s < nc ? h.h_prior[(o + n) * A + s] : 0.0;
      t.child(n, s) = ch;
      int sv = 0;
      double q = 0.0;
      if (ch >= 0) {
        t.parent_slot(ch) = s;
        sv = t.visit(ch);
        if (sv > 0) {
          const double v = t.value_sum(ch) / (double)sv;
          q = p.num_players == 1 ? t.reward(ch) + p.discount * v : t.reward(ch) + p.discount * (-v);
        }
      }
      t.slot_visit(n, s) = sv;
      t.slot_q(n, s) = q;
    }
  }
  return 0;
}

}  // namespace mzx
