// mzx_fused_fc2.h -- second generation of the whole-search kernel for fully connected networks
// (K5 of SURVEY.md section 8a): same contract as mzx_fused_fc.h -- initial_inference, root expansion and
// num_simulations x {select, recurrent_inference, expand, backpropagate} in ONE launch, every tree resident
// in LDS, bit-identical tree statistics to the generic path (mzx_tree.h) -- with the selection walk, which was
// 46 % of a simulation, rebuilt around what actually changes between two visits of a node.
//
// Reference semantics: MCTS.run /root/reference/self_play.py:260-361, ucb_score :380-404,
// backpropagate :406-430, MinMaxStats :553-570.
//
//   ucb_score(parent, child) = pb_c(N, n) * prior  +  [n > 0] normalize(reward + discount * (+-value))
//
//   * prior score  ps = (pbc[N] * (sqrt[N] / (n + 1))) * prior  depends on the parent's visit count N and the
//     child's n only: it changes exactly for the slots of the nodes on the path just back-propagated.  It is
//     CACHED per child slot and refreshed right after back-propagation by the lane that owns the path node
//     (N is in its registers), A slots per lane.  The walk no longer evaluates it: no table look-ups chained
//     behind the slot read, no division.
//   * value score  normalize(q) = (q - min) / (max - min)  depends on the tree-wide MinMaxStats, which move in
//     about every second simulation -- it cannot be cached, but its DIVISOR is the same for every node of a
//     simulation.  hipcc expands a binary64 division into div_scale, rcp, two Newton steps on the reciprocal,
//     then mul / fma / div_fmas / div_fixup on the numerator (AMDGPU LowerFDIV64); the first half depends on the
//     divisor only and is hoisted out of the walk (`recip_refined`, once per simulation); per child remain
//     mul, fma, fma, div_fixup -- the SAME instructions on the same operands, hence the same bits.  (div_scale
//     is the identity unless an operand is denormal or the exponents differ by more than 2^9 orders of
//     magnitude: tree statistics are sums of at most num_simulations fp32-origin values, so neither occurs.)
//     The two divisions by small integers (sqrt[N] / (n + 1), value_sum / visit_count) use the same split with a
//     per-integer reciprocal table filled at kernel start by the same instructions.
//   * one LDS round trip per level: a child slot is ONE 32-byte record {prior score, q, visit count, child
//     link, prior}; for two-action games the argmax needs no wave ballot (both scores are broadcast in the row).
//   * the path of a walk is kept in an LDS array instead of "lane d remembers depth d", and back-propagation
//     runs over 16-level chunks of it: searches deeper than 16 plies no longer fall back to a serial lane.
//
// Mapping, network engines (SmallNet / LdsNet) and the canonical fp32 reduction order are those of
// mzx_fused_fc.h.  The trees are converted to the arena's TreeLayout on export (mode flag 2), so
// mzx_search_dump and the bit-identity tests see the same data as with the generic path.
#pragma once
#include "mzx_fused_fc.h"

namespace mzx {

struct Fc2Args {
  // roots the caller expanded itself (MCTS.run(..., override_root_with=root), self_play.py:275-277,
  // diagnose_model.py:57-74): hidden state / child priors in legal-action order / reward replace initial_inference
  const float* ov_hidden;    // [B][E]   (null: the kernel runs initial_inference)
  const double* ov_priors;   // [B][A]
  const double* ov_reward;   // [B]
  FusedFcArgs f;   // network description, search parameters, io, export pointers (f.L = arena TreeLayout)
  int32_t off_slots, off_nodes, off_path, off_roota, off_mm, off_hidden, off_scratch;  // byte offsets inside a tree's slab
  int32_t tree_stride, lds_inv;                                               // lds_inv: reciprocal table (bytes)
};

#ifndef MZX_HOSTCHECK

// One child slot of a node.  INVARIANT: every one of the AW slots of a node that exists is written when the node is made
// (root expansion, fc2_expand, fc2_from_arena) -- slots beyond its actions with n = 0, prior = 0, ps = -inf.
// fc2_load_lane reads all AW slots of a path node without asking how many actions there are.
struct __attribute__((aligned(16))) Fc2Slot {
  double ps;       // cached prior score of the slot at the parent's current visit count
  double q;        // reward + discount * (+-value()) of the child (written by back-propagation)
  int32_t n;       // child's visit count
  int32_t child;   // canonical node index or -1
  double prior;
};
struct __attribute__((aligned(16))) Fc2Node {
  double value_sum, reward;
  int32_t visit, to_play, parent, parent_slot;
};
static_assert(sizeof(Fc2Slot) == 32 && sizeof(Fc2Node) == 32, "record size");

// Divisor-only half of hipcc's binary64 division expansion: v_rcp_f64 + two Newton steps.
__device__ __forceinline__ double recip_refined(double b) {
  const double y0 = __builtin_amdgcn_rcp(b);
  const double f0 = __builtin_fma(-b, y0, 1.0);
  const double f1 = __builtin_fma(y0, f0, y0);
  const double f2 = __builtin_fma(-b, f1, 1.0);
  return __builtin_fma(f1, f2, f1);
}
// Numerator half: a / b given y = recip_refined(b).
__device__ __forceinline__ double div_by(double a, double b, double y) {
  const double m = a * y;
  const double r = __builtin_fma(-b, m, a);
  const double q = __builtin_fma(r, y, m);
  return __builtin_amdgcn_div_fixup(q, b, a);
}
// prior_score of ucb_score (self_play.py:384-392), operation order of ucb_from (mzx_tree.h)
__device__ __forceinline__ double prior_score(double pbcN, double sqN, int n, double inv_n1, double prior) {
  const double pb_c = pbcN * div_by(sqN, (double)(n + 1), inv_n1);
  return pb_c * prior;
}

// Butterflies over the first W lanes of a row (the other lanes hold the neutral element): the canonical
// order xor 1, xor 2, half-mirror, mirror cut after log2(W) steps -- the skipped steps would add zeros / compare
// with the neutral element, so the result has the same bits as the 16-lane form.  (row_max_w / row_min_w: mzx_fused_fc.h.)
template <int W>
__device__ __forceinline__ float row_sum_w(float v) {
  v = v + dpp_f<DPP_XOR1>(v);
  if constexpr (W > 2) v = v + dpp_f<DPP_XOR2>(v);
  if constexpr (W > 4) v = v + dpp_f<DPP_HALF_MIRROR>(v);
  if constexpr (W > 8) v = v + dpp_f<DPP_MIRROR>(v);
  return v;
}
constexpr int DPP_ROW_SHL1 = 0x101;   // lane i reads lane i + 1 of its row (lane 15: keeps `old`)
__device__ __forceinline__ int shl1_i(int v, int old) {
  return __builtin_amdgcn_update_dpp(old, v, DPP_ROW_SHL1, 0xF, 0xF, false);
}
__device__ __forceinline__ double shl1_d(double v, double old) {
  return __hiloint2double(shl1_i(__double2hiint(v), __double2hiint(old)), shl1_i(__double2loint(v), __double2loint(old)));
}

// One step of the value recurrence  value = (+-reward) + discount * value  (self_play.py:417 / :424-427) at path
// lane J.  Lane `sub` advances its own copy of the value while the step is below its row's leaf and above its own
// node (sub < J <= ld) and then stops: what it holds when the chain ends IS the value arriving at its node, and lane 0
// holds the row's final value.  Until a lane stops, its copy went through the same operations on the same operands as
// every other copy of the row, hence the same bits as one row-uniform value.  `lim` = max(ld - sub, 0): the condition
// is one unsigned compare of the lane constant J - 1 - sub against it -- a select, no exec-mask branch.
// The reward arrives as the DPP operand of the addition (add_bcast_d: `r_eff` at row_newbcast:J, `one` = 1.0 in registers):
// a step is mul, add, the compare of the step AFTER it, two selects -- with its own compare in front hipcc put an s_nop 0
// between the asm statement and the selects of every step; the next step's compare takes that slot.  The first compare of
// a group is made at its entry.  fc2_backprop readies `r_eff` for DPP reads once per chunk; no wait state per step.
template <int J>
__device__ __forceinline__ bool chain_on(unsigned lim, int sub) { return (unsigned)(J - 1 - sub) < lim; }
template <int J, bool NEXT>
__device__ __forceinline__ void chain_step2(double r_eff, double disc, double one, unsigned lim, int sub, bool& on, double& val) {
  const bool now = on;
  const double nv = add_bcast_d<J>(r_eff, disc * val, one);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NEXT) on = chain_on<J - 1>(lim, sub);
  __builtin_amdgcn_sched_barrier(0);
  val = now ? nv : val;
}
// The same step with the reward broadcast by a pair of 32-bit moves and a plain addition (7 instructions): the form of the
// instantiations that do not take 64-bit DPP operands (D64 = false below).
template <int J>
__device__ __forceinline__ void chain_step2_moves(double r_eff, double disc, unsigned lim, int sub, double& val) {
  const bool on = chain_on<J>(lim, sub);
  __builtin_amdgcn_sched_barrier(0);
  const double rj = bcast_d<J>(r_eff);
  const double nv = rj + disc * val;
  val = on ? nv : val;
}
template <bool D64, int J, bool NEXT>
__device__ __forceinline__ void chain_step(double r_eff, double disc, double one, unsigned lim, int sub, bool& on, double& val) {
  if constexpr (D64) chain_step2<J, NEXT>(r_eff, disc, one, lim, sub, on, val);
  else chain_step2_moves<J>(r_eff, disc, lim, sub, val);
}
// Steps 15 .. 7 in three groups guarded by the deepest row of the wave (wmax, wave-uniform: plain scalar branches, no
// exec masking); a step above a row's own leaf is a no-op by its select, so a group may run a step too many.
template <bool D64>
__device__ __forceinline__ void value_chain(double r_eff, double disc, double one, int ld, int sub, int wmax, double& val) {
  const int room = ld - sub;
  const unsigned lim = (unsigned)(room > 0 ? room : 0);
  bool on6 = chain_on<6>(lim, sub);          // ahead of the guarded groups: ready when step 6 selects
  if (wmax >= 13) {
    bool on = chain_on<15>(lim, sub);
    chain_step<D64, 15, true>(r_eff, disc, one, lim, sub, on, val);
    chain_step<D64, 14, true>(r_eff, disc, one, lim, sub, on, val);
    chain_step<D64, 13, false>(r_eff, disc, one, lim, sub, on, val);
  }
  if (wmax >= 9) {
    bool on = chain_on<12>(lim, sub);
    chain_step<D64, 12, true>(r_eff, disc, one, lim, sub, on, val);
    chain_step<D64, 11, true>(r_eff, disc, one, lim, sub, on, val);
    chain_step<D64, 10, true>(r_eff, disc, one, lim, sub, on, val);
    chain_step<D64, 9, false>(r_eff, disc, one, lim, sub, on, val);
  }
  if (wmax >= 7) {
    bool on = chain_on<8>(lim, sub);
    chain_step<D64, 8, true>(r_eff, disc, one, lim, sub, on, val);
    chain_step<D64, 7, false>(r_eff, disc, one, lim, sub, on, val);
  }
  // steps 6 .. 1 without a guard: of the waves of a C2 search (4096 trees x 50 simulations) 71 % reach depth 5 and 50 %
  // depth 6; a compare-and-branch pair per step cost more than the steps a shallow wave now runs for nothing
  chain_step<D64, 6, true>(r_eff, disc, one, lim, sub, on6, val);
  chain_step<D64, 5, true>(r_eff, disc, one, lim, sub, on6, val);
  chain_step<D64, 4, true>(r_eff, disc, one, lim, sub, on6, val);
  chain_step<D64, 3, true>(r_eff, disc, one, lim, sub, on6, val);
  chain_step<D64, 2, true>(r_eff, disc, one, lim, sub, on6, val);
  chain_step<D64, 1, false>(r_eff, disc, one, lim, sub, on6, val);
}


// ---------------------------------------------------------------------------
// The tree side of one simulation as row-collective functions over LDS records (one 16-lane row per tree): used by
// the fully connected kernel below and by the residual whole-search kernel (mzx_resnet_search.h) when its trees
// are LDS-resident.

struct Fc2Tree {              // LDS views of one tree + the workgroup's tables
  Fc2Slot* slots;             // [NN][AW]
  Fc2Node* nodes;             // [NN]
  int2* path;                 // [NN + 1]: {node at depth d, slot taken from its parent}
  int32_t* roota;             // [AW]: action of root slot s
  double* mm;                 // MinMaxStats {minimum, maximum}: updated by LDS min / max
  const double *pbc, *sqt, *inv_y;
  double pb_leaf, disc;       // pb_c(N = 1, n = 0): prior-score factor of a fresh leaf's slots
  int A, NN, P;
};
struct Fc2Row { int32_t n_nodes, tape_pos, flags, ties, max_depth, sum_depth, root_n, root_to_play; };
struct Fc2Walk { int parent, slot, leaf, depth, levels, vtp, action; };

// Selection walk (self_play.py:325-334, :363-404).  Slots that do not exist (root slots beyond the legal actions,
// padding up to AW) carry a prior score of -inf and n = 0, so their score is -inf without a validity test.  A row
// that has reached its leaf keeps executing with its state frozen (one straight-line body per level per wave).
template <int AW>
__device__ __forceinline__ Fc2Walk fc2_walk(const Fc2Tree& T, Fc2Row& st, const uint32_t* tape, int tape_words, int sub,
                                            int row_in_wave) {
  const double2 mmv = *(const double2*)T.mm;   // MinMaxStats after the previous back-propagation
  const double mn = mmv.x, mx = mmv.y;
  const double dd = mx - mn;                 // MinMaxStats.normalize divisor, same for every node of this walk
  const double yd = recip_refined(dd);       // (garbage while max <= min: results discarded like the reference's branch)
  const bool norm_on = mx > mn;
  int node = 0, depth = 0, slot = 0;
  int levels = 0;                  // walk iterations = depth of the deepest leaf in this wave (scalar)
  if constexpr (AW == 2) {
    // Two candidates: every lane sees both scores, no ballot.  One loop counter, one backward conditional branch.
    // While max <= min the reference takes q as it is: with minimum 0 and divisor 1 the division returns q bit for
    // bit ((q - 0) * 1, a zero remainder, div_fixup(q, 1, q) = q), so the select is made once per walk, not per level.
    const double mn_e = norm_on ? mn : 0.0, dd_e = norm_on ? dd : 1.0, yd_e = norm_on ? yd : 1.0;
    unsigned long long more = __builtin_amdgcn_ballot_w64(true);   // lanes whose row has not reached its leaf
    do {
      const bool act = __builtin_amdgcn_inverse_ballot_w64(more);
      ++levels;
      asm volatile("" : "+s"(levels));      // one induction variable (the compiler kept three copies of it)
      const Fc2Slot* rp = T.slots + (node * 2 + (sub & 1));
      const double ps = rp->ps, q = rp->q;
      const int n = rp->n, c = rp->child;
      const bool seen = n > 0;
      __builtin_amdgcn_sched_barrier(0);    // the compare first: the division fills its wait states before the select
      const double v = div_by(q - mn_e, dd_e, yd_e);
      const double wv = ps + v;
      const double sc = seen ? wv : ps;
      const int c0 = bcast_i<0>(c), c1 = bcast_i<1>(c);     // ahead of the scores: two wait states behind sc's select
      const double a0 = bcast_d64<0>(sc), a1 = bcast_d64<1>(sc);
      const bool up = a1 > a0;     // the child is selected by the comparison itself
      int sl = up ? 1 : 0;
      int cw = up ? c1 : c0;
      const bool eq = a0 == a1;
      if (__builtin_expect((__builtin_amdgcn_ballot_w64(eq) & more) != 0, 0)) {   // wave-uniform: a scalar branch, no exec round trip
        if (eq && act) {           // numpy.random.choice([0, 1]): first walk of a search, rare later
          ++st.ties;
          sl = tape_draw(tape, tape_words, st.tape_pos, st.flags, 2);
          cw = sl ? c1 : c0;
        }
      }
      cw = act ? cw : -1;          // a finished row has no child to go to: `cw >= 0` alone says "walk on"
      // entry of the level just decided; a finished row rewrites the entry beyond its leaf (never read)
      T.path[depth + 1] = make_int2(cw, sl);      // row-uniform address and value: every lane of the row stores it
      depth += act ? 1 : 0;
      asm volatile("" : "+v"(depth));
      slot = act ? sl : slot;
      const bool go = cw >= 0;
      node = go ? cw : node;
      more = __builtin_amdgcn_ballot_w64(go);
    } while (more != 0);
  } else {
  bool done = false;
  for (;;) {
    ++levels;
    const Fc2Slot* rp = T.slots + (node * AW + (sub & (AW - 1)));
    const double ps = rp->ps, q = rp->q;
    const int n = rp->n, c = rp->child;
    const double nv = div_by(q - mn, dd, yd);
    const double v = norm_on ? nv : q;
    const double wv = ps + v;
    const double sc = (n > 0) ? wv : ps;
    int sl, cw;
    {
      const double best = row_max_d<AW>(sc);
      const unsigned bits = row_bits(__ballot(sc == best), row_in_wave) & ((1u << AW) - 1u);
      const int nbest = __popc(bits);
      sl = nbest ? (__ffs(bits) - 1) : 0;
      if (__builtin_expect(nbest > 1 && !done, 0)) {  // numpy.random.choice(ties): k-th maximiser in slot order
        ++st.ties;
        int k = tape_draw(tape, tape_words, st.tape_pos, st.flags, nbest);
        unsigned b = bits;
        for (; k > 0; --k) b &= b - 1;
        sl = __ffs(b) - 1;
      }
      if constexpr (AW <= 4) cw = pick_i<AW>(c, sl);
      else cw = perm_i(c, sl, row_in_wave);
    }
    const bool act = !done;
    cw = act ? cw : -1;              // a finished row has no child to go to: `cw >= 0` alone says "walk on"
    // entry of the level just decided; a finished row rewrites the entry beyond its leaf (never read)
    T.path[depth + 1] = make_int2(cw, sl);       // row-uniform address and value: every lane of the row stores it
    depth += act ? 1 : 0;
    slot = act ? sl : slot;
    const bool go = cw >= 0;
    node = go ? cw : node;
    done = !go;
    if (__builtin_amdgcn_ballot_w64(go) == 0) break;   // __all(done), as a ballot of the comparison itself
  }
  }
  Fc2Walk w;
  // players play turn by turn (self_play.py:331-334): the leaf's player follows from the depth
  w.vtp = (T.P == 1) ? 0 : ((st.root_to_play + depth) & 1);
  int leaf = st.n_nodes;
  if (leaf >= T.NN) { st.flags |= TF_NODE_OVERFLOW; leaf = T.NN - 1; }
  T.path[depth] = make_int2(leaf, slot);         // by the whole row, like the entries of the levels above
  const int ra = T.roota[slot < AW ? slot : 0];
  w.parent = node; w.slot = slot; w.leaf = leaf; w.depth = depth; w.levels = levels;
  w.action = (node == 0) ? ra : slot;
  return w;
}

// What back-propagation needs about the path node a lane owns (lane j of chunk c <-> depth 16 c + j).
template <int AW>
struct Fc2Lane {
  int nd, pslot, par, vc, tp, rpar;    // rpar: the `parent` field the lane's node record keeps (root: -1)
  double vs, rr, inv_vc2, inv_vc3, pb, sv;
  int sn[AW <= 4 ? AW : 1];
  double sprior[AW <= 4 ? AW : 1], sinv[AW <= 4 ? AW : 1];
};

// Everything back-propagation needs from the tree is independent of the network: fetched BEFORE it, so that the
// LDS latency hides behind recurrent_inference.  (Call after a wave_sync following fc2_walk.)
template <int AW>
__device__ __forceinline__ Fc2Lane<AW> fc2_load_lane(const Fc2Tree& T, const Fc2Walk& w, int c, int sub) {
  Fc2Lane<AW> L;
  const int d = c * 16 + sub;
  // No guard on a READ: a lane at or beyond the leaf reads the leaf's path entry and, for the node record, the leaf's
  // parent -- a real record, so every count below indexes its table in range.  Such a lane ends up with the LEAF's operands
  // (path entry, value_sum = 0, visit = 0, the walk's player): back-propagation computes the leaf's record in it once more and
  // stores it to the leaf's address again (fc2_backprop), so no write needs a guard either.
  const bool inner = d < w.depth;
  const int dq = inner ? d : w.depth;
  const int2 pe = T.path[dq];
  L.nd = pe.x; L.pslot = pe.y;
  L.par = T.path[dq > 0 ? dq - 1 : 0].x;     // (depth >= 1: a walk takes at least the root's level)
  const int nr = inner ? L.nd : L.par;
  const Fc2Node* np = T.nodes + nr;
  const double vs = np->value_sum;
  const int4 hv = *(const int4*)&np->visit;   // {visit, to_play, parent, parent_slot}: the record's second half in one read
  L.rr = np->reward;   // (at and beyond the leaf: the parent's reward -- back-propagation replaces it by the leaf's)
  L.vs = inner ? vs : 0.0; L.vc = inner ? hv.x : 0;
  L.tp = inner ? hv.y : w.vtp;           // written back with the record; one player: compared by nobody
  L.rpar = inner ? hv.z : L.par;         // the root keeps its -1 (its path entry names node 0 as its own parent)
  L.inv_vc2 = T.inv_y[L.vc + 1];        // reciprocal of this node's visit count after the update
  L.inv_vc3 = T.inv_y[L.vc + 2];        // ... and of (that + 1): what its PARENT's prior score divides by
  L.pb = T.pbc[L.vc + 1]; L.sv = T.sqt[L.vc + 1];
  if constexpr (AW <= 4) {
    // all AW slots of a real node are initialised (padding slots: n = 0, prior = 0)
#pragma unroll
    for (int s = 0; s < AW; ++s) { L.sn[s] = T.slots[nr * AW + s].n; L.sprior[s] = T.slots[nr * AW + s].prior; }
#pragma unroll
    for (int s = 0; s < AW; ++s) L.sinv[s] = T.inv_y[L.sn[s] + 1];
  }
  return L;
}

// Node.expand (self_play.py:451-465): child slot `sub` of the new leaf (lanes < AW; `in`: the slot exists).  Whole rows only.
template <int AW>
__device__ __forceinline__ void fc2_expand(const Fc2Tree& T, int leaf, int sub, bool in, double prior) {
  Fc2Slot s;
  s.prior = in ? prior : 0.0;
  s.q = 0.0; s.n = 0; s.child = -1;
  s.ps = in ? T.pb_leaf * s.prior : -MZX_INF;   // prior score once the leaf has its first visit (N = 1, n = 0)
  // no exec mask: the lanes beyond the record lanes store into the tree's dead slot row ("node -1", see fc2_plan)
  static_assert(AW <= 4 || AW == FUSED_ROW, "a dead slot row exists for 2- and 4-lane records only");
  int at = leaf * AW + sub;
  if constexpr (AW < FUSED_ROW) at = (sub < AW) ? at : -AW;
  T.slots[at] = s;
}

// MCTS.backpropagate (self_play.py:406-430) + refresh of the cached prior scores along the path.  `L` = the
// lane's operands of chunk w.levels >> 4 (fc2_load_lane before the network).
template <int AW>
__device__ __forceinline__ void fc2_backprop(const Fc2Tree& T, Fc2Row& st, const Fc2Walk& w, Fc2Lane<AW> L, int sub,
                                             double value, double reward) {
  static_assert(AW <= 4 || AW == FUSED_ROW, "a dead slot row exists for 2- and 4-lane records only");
  const int depth = w.depth, vtp = w.vtp, P = T.P;
  const double disc = T.disc;
  st.n_nodes = w.leaf + 1;
  if (depth > st.max_depth) st.max_depth = depth;
  st.sum_depth += depth;
  const int cmax = w.levels >> 4;    // wave-uniform number of 16-level chunks - 1 (0 unless a path is > 15 deep)
  double val = value;
  int carry_vc2 = 0, carry_pslot = -1;       // lane 0 of the chunk below (deeper), for lane 15 of this one
  double carry_inv = 0.0;
  constexpr bool D64 = (AW == 2);            // 64-bit DPP operands: the two-action instantiations (see bcast_d64)
  const double one = 1.0;                    // register operand of add_bcast_d
  for (int c = cmax; c >= 0; --c) {
    if (c != cmax) { wave_sync(); L = fc2_load_lane<AW>(T, w, c, sub); }
    const int d = c * 16 + sub;
    const int ld = depth - c * 16;             // row-uniform: depth of the leaf relative to this chunk
    const bool inner = d < depth;               // lanes at AND beyond the leaf carry the leaf's operands (fc2_load_lane)
    const double rr = inner ? L.rr : reward;
    const bool same = (L.tp == vtp);
    // value = (+-reward) + discount * value; the selects that make it are VALU writes: two wait states once, ahead of
    // every DPP read of it below (the chain's steps and the hand-over)
    const double r_sel = (P == 1 || !same) ? rr : -rr;
    const double r_eff = D64 ? dpp_ready_d(r_sel) : r_sel;
    const int wm = w.levels - c * 16;           // deepest leaf of the wave relative to this chunk (wave-uniform)
    value_chain<D64>(r_eff, disc, one, ld, sub, wm > 15 ? 15 : (wm < 0 ? 0 : wm), val);
    const double my_in = val;                   // the value arriving at this lane's node (lane 0: the chunk's final value)
    // hand the value to the chunk above: lane 0's, through lane 0's node -- row-uniform again.  Behind a scalar branch:
    // the first chunk of a search no deeper than 15 plies (c == 0) issues none of it.
    if (c > 0) {
      double nv;
      if constexpr (D64) nv = add_bcast_d<0>(r_eff, disc * bcast_d64<0>(val), one);
      else nv = bcast_d<0>(r_eff) + disc * bcast_d<0>(val);
      val = (ld >= 0) ? nv : val;
    }
    const int vc2 = L.vc + 1;
    const double vs2 = L.vs + ((P == 1 || same) ? my_in : -my_in);
    // No store below has a guard (2- and 4-lane records).  An inner lane stores its own node; the lanes at and beyond the
    // leaf ALL hold the leaf's operands and store the leaf's record, link and slot statistics -- the same values to the
    // same addresses, as the walk stores a path entry.  The root lane has no parent slot: its {q, n, child} land in
    // slot -1, the last record of the dead slot row in front of the tree's slots (fc2_plan), which nothing reads.
    const double mean = div_by(vs2, (double)vc2, L.inv_vc2);
    const double qv = rr + disc * ((P == 1) ? mean : -mean);
    {
      Fc2Node r;
      r.value_sum = vs2; r.reward = rr; r.visit = vc2; r.to_play = L.tp; r.parent = L.rpar; r.parent_slot = L.pslot;
      T.nodes[L.nd] = r;
      // 16-lane records have no dead row (512 bytes a tree: a plan at the LDS budget no longer fitted);
      // there the root lane is masked off
      if (AW <= 4 || d > 0) {
        Fc2Slot* ps = T.slots + (L.par * AW + L.pslot);
        ps->q = qv;
        *(int2*)&ps->n = make_int2(vc2, L.nd);     // {n, child}: the link is rewritten (inner node) or made (leaf)
      }
      // MinMaxStats.update (self_play.py:562-564): pure min / max over the path nodes, order-free.  The one guard that
      // stays: LDS atomics of several lanes on ONE address are served lane after lane, and the ten or so lanes beyond
      // the leaf repeating the leaf's value cost 9 % of the launch (profiles/fc2_tree_writes_ab.txt).
      if (d <= depth) {
        __hip_atomic_fetch_min(&T.mm[0], qv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_max(&T.mm[1], qv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    // prior scores of this node's child slots at its new visit count N = vc2 (see header).  The slot on the
    // path just received the child's new visit count: taken from the lane above instead of LDS.
    if constexpr (AW <= 4) {
      const int ch_vc2 = shl1_i(vc2, carry_vc2), ch_slot = shl1_i(L.pslot, carry_pslot);
      const double ch_inv = shl1_d(L.inv_vc3, carry_inv);
      // unconditional: a lane without an inner node aims at the dead slot row; a slot beyond the node's actions holds
      // -inf and receives -inf
      const int nslots = (L.nd == 0) ? st.root_n : T.A;
      Fc2Slot* sp = T.slots + (inner ? L.nd : -1) * AW;
#pragma unroll
      for (int s = 0; s < AW; ++s) {
        const bool on_path = (s == ch_slot);
        const int ns = on_path ? ch_vc2 : L.sn[s];
        const double iv = on_path ? ch_inv : L.sinv[s];
        const double psc = prior_score(L.pb, L.sv, ns, iv, L.sprior[s]);
        sp[s].ps = (s < nslots) ? psc : -MZX_INF;
      }
      carry_vc2 = bcast_i<0>(vc2); carry_pslot = bcast_i<0>(L.pslot); carry_inv = D64 ? bcast_d64<0>(L.inv_vc3) : bcast_d<0>(L.inv_vc3);
    } else {
      wave_sync();
      if (inner) {
        Fc2Slot* sp = T.slots + L.nd * AW;
        const int nslots = (L.nd == 0) ? st.root_n : T.A;
        for (int s = 0; s < nslots; ++s) {
          const int ns = sp[s].n;
          sp[s].ps = prior_score(L.pb, L.sv, ns, T.inv_y[ns + 1], sp[s].prior);
        }
      }
    }
  }
  wave_sync();
}

// Arena tree (TreeLayout) -> the slot / node records above in LDS: a root RootInitOp left alone (the residual whole-search
// kernel, mzx_resnet_search.h), or a carried tree ContinueRootOp prepared (fc2_search_kernel's continued searches).  The
// cached prior score of every slot is recomputed at its node's visit count with prior_score -- the operations of the
// refresh after back-propagation, hence the bits a tree grown in LDS would hold.  Called by the 16-lane row of the tree.
template <int RW>
__device__ __forceinline__ void fc2_from_arena(const Fc2Tree& FT, Fc2Row& rst, const TreeRef& t, int sub) {
  const int nn = t.meta(TM_N_NODES), rootn = t.meta(TM_ROOT_N);
  for (int n = sub; n < nn; n += FUSED_ROW) {
    Fc2Node r;
    r.value_sum = t.value_sum(n); r.reward = t.reward(n); r.visit = t.visit(n); r.to_play = t.to_play(n);
    r.parent = t.parent(n); r.parent_slot = t.parent_slot(n);
    FT.nodes[n] = r;
    const int nc = (n == 0) ? rootn : FT.A;
    for (int s2 = 0; s2 < RW; ++s2) {
      Fc2Slot q;
      const bool in = s2 < nc;
      q.prior = in ? t.prior(n, s2) : 0.0; q.q = in ? t.slot_q(n, s2) : 0.0;
      q.n = in ? t.slot_visit(n, s2) : 0; q.child = in ? t.child(n, s2) : -1;
      q.ps = in ? prior_score(FT.pbc[r.visit], FT.sqt[r.visit], q.n, FT.inv_y[q.n + 1], q.prior) : -MZX_INF;
      FT.slots[n * RW + s2] = q;
    }
  }
  if (sub < RW) FT.roota[sub] = (sub < rootn) ? t.root_action(sub) : -1;
  if (sub == 0) { FT.path[0] = make_int2(0, -1); FT.mm[0] = t.mm_min(); FT.mm[1] = t.mm_max(); }
  rst.n_nodes = nn; rst.tape_pos = t.meta(TM_TAPE_POS); rst.flags = t.meta(TM_FLAGS); rst.ties = t.meta(TM_TIE_DRAWS);
  rst.max_depth = t.meta(TM_MAX_DEPTH); rst.sum_depth = t.meta(TM_SUM_DEPTH); rst.root_n = rootn;
  rst.root_to_play = t.to_play(0);
}

// CONT: a continued search (mzx_tree_carry.h) -- each tree comes from the arena (f.export_trees / f.export_hidden, where
// mzx_search_advance / mzx_search_load put it and ContinueRootOp prepared its root) instead of initial_inference and root
// expansion; continued simulation k expands node n_carried + k, the root's N is its visit count from the tree, and the
// grown tree goes back to the same place.  CONT = false is the fresh search, unchanged.
template <class Net, int AW, bool PROFILE, bool CONT = false>
__global__ void __launch_bounds__(256) fc2_search_kernel(const Fc2Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int sub = tid & (FUSED_ROW - 1);
  const int row = tid / FUSED_ROW;
  const int row_in_wave = row & 3;
  const int tree = blockIdx.x * a.f.trees_per_block + row;
  const int A = a.f.p.num_actions, E = a.f.E, NN = a.f.p.num_nodes, P = a.f.p.num_players;
  const double disc = a.f.p.discount;
  uint32_t prof[FUSED_PROF_WORDS];
  unsigned long long t_last = 0;
  if (PROFILE) {
    for (int k = 0; k < FUSED_PROF_WORDS; ++k) prof[k] = 0;
    t_last = __builtin_readcyclecounter();
  }

  // ---- every global input of the launch is requested HERE, back to back, and waited for once ("Launch
  // prologue"): the thread's table entry, the lane's weight rows and the tree's observation (Net::request), its legal
  // action, player and noise, or the caller's root (OVERRIDE).  A continued search takes its root from the arena: tables
  // and weights only.  The exit below comes AFTER these reads, so they index a clamped tree: a row that will exit reads
  // the inputs of the launch's last tree and drops them (the row itself is below trees_per_block: the launch has
  // trees_per_block rows of threads); a lane beyond A or E reads the row's last entry.
  const int ntab = 2 * (NN + 1);
  const double tab_r = a.f.tables[tid < ntab ? tid : ntab - 1];
  const int tree_c = tree < a.f.p.num_trees ? tree : a.f.p.num_trees - 1;
  const bool given = !CONT && a.ov_hidden != nullptr;   // (launch-uniform) the caller's roots: no initial_inference
  const bool noisy = a.f.io.d_noise != nullptr;         // (launch-uniform)
  Net net;
  net.request(a.f, sub, a.f.io.d_observation + (size_t)tree_c * a.f.in_size, !CONT && !given);
  int32_t lg_r = -1, tp_r = 0;
  double nz_r = 0.0, ovp_r = 0.0, ovr_r = 0.0;
  float ovh_r = 0.f;
  if constexpr (!CONT) {
    const int ac = sub < A ? sub : A - 1;
    lg_r = a.f.io.d_legal_actions[(size_t)tree_c * A + ac];
    tp_r = a.f.io.d_to_play[tree_c];
    if (noisy) nz_r = a.f.io.d_noise[(size_t)tree_c * A + ac];
    if (given) {
      ovh_r = a.ov_hidden[(size_t)tree_c * E + (sub < E ? sub : E - 1)];
      ovp_r = a.ov_priors[(size_t)tree_c * A + ac];
      ovr_r = a.ov_reward[tree_c];
    }
  }

  // ---- stage tables (+ weights): the only workgroup-wide barrier.  The reciprocals are arithmetic behind the requests.
  double* tables = (double*)(smem + a.f.lds_tables);
  double* inv_y = (double*)(smem + a.lds_inv);   // [NN + 2]: refined reciprocal of the integer k >= 1
  for (int i = tid; i < NN + 2; i += blockDim.x) inv_y[i] = recip_refined((double)(i > 0 ? i : 1));
  net.stage(a.f, smem, tid);
  // The launch's one wait for global memory, as the instruction itself (vmcnt(0), the other counters left alone): the
  // compiler's own wait insertion reads it, so no load above is waited for again at its first use -- which for most of
  // the weight rows is inside the simulation loop, an issue slot per wait and simulation.  The empty statement pins the
  // requests of this function above it.
  __builtin_amdgcn_s_waitcnt(0x0F70);
  asm volatile("" ::"v"(tab_r), "v"(lg_r), "v"(tp_r), "v"(nz_r), "v"(ovp_r), "v"(ovr_r), "v"(ovh_r));
  if (tid < ntab) tables[tid] = tab_r;
  for (int i = tid + blockDim.x; i < ntab; i += blockDim.x) tables[i] = a.f.tables[i];   // more entries than threads
  __syncthreads();
  if (row >= a.f.trees_per_block || tree >= a.f.p.num_trees) return;  // whole rows exit together
  net.attach(a.f, smem);
  const double* pbc = tables;
  const double* sqt = tables + (NN + 1);
  // prior-score factor of a freshly expanded leaf's slots: the leaf has ONE visit after its own
  // back-propagation and its children none -- pb_c(N = 1, n = 0)
  const double pb_leaf = pbc[1] * div_by(sqt[1], 1.0, inv_y[1]);

  char* slab = smem + a.f.lds_trees + (size_t)row * a.tree_stride;
  Fc2Slot* slots = (Fc2Slot*)(slab + a.off_slots);   // [NN][AW]
  Fc2Node* nodes = (Fc2Node*)(slab + a.off_nodes);   // [NN]
  int2* path = (int2*)(slab + a.off_path);           // [NN + 1]: {node at depth d, slot taken from its parent}
  int32_t* roota = (int32_t*)(slab + a.off_roota);   // [AW]: action of root slot s
  double* mm = (double*)(slab + a.off_mm);           // MinMaxStats {minimum, maximum}: updated by LDS min / max
  float* hidden = (float*)(slab + a.off_hidden);     // [NN][E]
  float* scr = (float*)(slab + a.off_scratch);
  const uint32_t* tape = (const uint32_t*)a.f.io.d_tape + (size_t)tree * a.f.p.tape_words;
  const int tape_words = a.f.p.tape_words;

  // per-tree scalars, row-uniform registers
  int32_t n_nodes = 1, tape_pos = 0, flags = 0, ties = 0, max_depth = 0, sum_depth = 0, root_n = 0, root_to_play = 0;
  MZX_PROF(0)

  // ---- a carried tree: node and slot records (prior scores recomputed), MinMaxStats, root actions and counters, and
  // the hidden state of every node, arena -> LDS
  if constexpr (CONT) {
    Fc2Tree FT;
    FT.slots = slots; FT.nodes = nodes; FT.path = path; FT.roota = roota; FT.mm = mm;
    FT.pbc = pbc; FT.sqt = sqt; FT.inv_y = inv_y; FT.A = A;
    TreeRef t;
    t.base = a.f.export_trees + (size_t)tree * a.f.L.tree_bytes;
    t.L = a.f.L;
    Fc2Row rst;
    fc2_from_arena<AW>(FT, rst, t, sub);
    n_nodes = rst.n_nodes; tape_pos = rst.tape_pos; flags = rst.flags; ties = rst.ties; max_depth = rst.max_depth;
    sum_depth = rst.sum_depth; root_n = rst.root_n; root_to_play = rst.root_to_play;
    const float* hd = a.f.export_hidden + (size_t)tree * NN * E;
    for (int i = sub; i < n_nodes * E; i += FUSED_ROW) hidden[i] = hd[i];
    wave_sync();
  }
  // ---- initial_inference (models.py:172-190) + root expansion (self_play.py:286-314, :467-476)
  if constexpr (!CONT) {
    NetOut o;
    if (!given) net.initial_requested(a.f.io.d_observation + (size_t)tree * a.f.in_size, hidden, scr, sub, o);
    else {
      if (sub < E) hidden[sub] = ovh_r;
      for (int e = sub + FUSED_ROW; e < E; e += FUSED_ROW) hidden[e] = a.ov_hidden[(size_t)tree * E + e];
    }
    // Root actions: the leading non-negative entries of the legal-action row, lane s holding entry s.  The serial scan
    // `while (n < A && lg[n] >= 0) ++n` stops at the FIRST s with s == A or lg[s] < 0; bit s of the row's ballot is set
    // exactly when s < A and lg[s] >= 0, so that s is the lowest clear bit -- the count of trailing ones -- whatever
    // follows it (a negative entry with non-negative ones behind it ends the count as it ends the scan).  Bits 16 and
    // up of the complement are set: the count is at most 16.
    root_n = __builtin_ctz(~row_bits(__ballot(sub < A && lg_r >= 0), row_in_wave));
    if (!given && sub < A) scr[sub] = o.policy;
    wave_sync();
    const bool in = sub < root_n;
    const float l = (in && !given) ? scr[lg_r] : -MZX_INF;   // logits gathered in the game's legal-action order
    const float m = row_max_w<AW>(l);
    const float e = (in && !given) ? mzx_expf(l - m) : 0.f;
    const float den = row_sum_w<AW>(e);
    root_to_play = tp_r;
    if (sub == 0) {
      Fc2Node r;
      r.value_sum = 0.0; r.visit = 0; r.to_play = root_to_play;
      r.reward = given ? ovr_r : (double)support_inverse_transform(0.0f);
      r.parent = -1; r.parent_slot = -1;
      nodes[0] = r;
      path[0] = make_int2(0, -1);
      mm[0] = MZX_INF; mm[1] = -MZX_INF;      // MinMaxStats (self_play.py:558-560)
      if (!given && a.f.io.d_root_predicted_value) a.f.io.d_root_predicted_value[tree] = (double)o.value;
    }
    if (sub < AW) {
      Fc2Slot s;
      const double pr = !in ? 0.0 : (given ? ovp_r : (double)mzx_div(e, den));
      s.prior = in ? root_noisy_prior(pr, noisy ? &nz_r : nullptr, 0, a.f.p.exploration_fraction) : 0.0;   // nz_r: this slot's noise
      s.q = 0.0; s.n = 0; s.child = -1;
      s.ps = in ? prior_score(pbc[0], sqt[0], 0, inv_y[1], s.prior) : -MZX_INF;   // root visit count 0
      slots[sub] = s;
      roota[sub] = in ? lg_r : -1;
    }
    wave_sync();
  }
  MZX_PROF(1)

  // ---- simulations (self_play.py:319-355)
  Fc2Tree T;
  T.slots = slots; T.nodes = nodes; T.path = path; T.roota = roota; T.mm = mm;
  T.pbc = pbc; T.sqt = sqt; T.inv_y = inv_y; T.pb_leaf = pb_leaf; T.disc = disc; T.A = A; T.NN = NN; T.P = P;
  Fc2Row st;
  st.n_nodes = n_nodes; st.tape_pos = tape_pos; st.flags = flags; st.ties = ties; st.max_depth = max_depth;
  st.sum_depth = sum_depth; st.root_n = root_n; st.root_to_play = root_to_play;
  const int num_sims = a.f.p.num_sims;
  // The loop's code starts a fixed distance behind a 64-byte boundary (the directive pads with s_nop, run once), so its
  // place no longer moves with the length of the prologue above.  A lone wave pays for where its branch targets lie in
  // the fetch lines: the SAME loop shifted in steps of 4 bytes measured 1.79 to 1.88 G simulations/s on C2, and this
  // change's shorter prologue had moved it from a good place to a bad one ("Launch prologue").
  asm volatile(".p2align 6");
  for (int sim = 0; sim < num_sims; ++sim) {
    const Fc2Walk w = fc2_walk<AW>(T, st, tape, tape_words, sub, row_in_wave);
    MZX_PROF(2)
    wave_sync();
    const Fc2Lane<AW> L = fc2_load_lane<AW>(T, w, w.levels >> 4, sub);
    MZX_PROF(7)

    // ------------------------------------------------------------- recurrent_inference (models.py:192-195)
    NetOut o;
    net.recurrent(hidden + w.parent * E, w.action, hidden + w.leaf * E, scr, sub, o);
    MZX_PROF(3)

    // ------------------------------------------------------------- expand (self_play.py:451-465)
    {
      const bool in = sub < A;
      const float m = row_max_w<AW>(in ? o.policy : -MZX_INF);
      const float e = in ? mzx_expf(o.policy - m) : 0.f;
      const float den = row_sum_w<AW>(e);
      fc2_expand<AW>(T, w.leaf, sub, in, (double)mzx_div(e, den));
    }
    MZX_PROF(4)

    // ------------------------------------------------------------- backpropagate (self_play.py:406-430)
    fc2_backprop<AW>(T, st, w, L, sub, (double)o.value, (double)o.reward);
    MZX_PROF(5)
  }
  n_nodes = st.n_nodes; tape_pos = st.tape_pos; flags = st.flags; ties = st.ties; max_depth = st.max_depth;
  sum_depth = st.sum_depth;

  // ---- results (FinalizeOp)
  if constexpr (AW <= 4) {
    // each action's count written once, by the lane of that action: the count of the root slot that holds it (the last
    // such slot, as the loop below would leave it), or zero.  roota is -1 beyond the root's slots.
    if (sub < A) {
      int c = 0;
#pragma unroll
      for (int s = 0; s < AW; ++s) c = (roota[s] == sub) ? slots[s].n : c;
      a.f.io.d_visit_counts[(size_t)tree * A + sub] = c;
    }
  }
  if (sub == 0) {
    if constexpr (AW > 4) {
      for (int x = 0; x < A; ++x) a.f.io.d_visit_counts[(size_t)tree * A + x] = 0;
      for (int s = 0; s < root_n; ++s) a.f.io.d_visit_counts[(size_t)tree * A + roota[s]] = slots[s].n;
    }
    const int vc = nodes[0].visit;
    a.f.io.d_root_value[tree] = (vc == 0) ? 0.0 : nodes[0].value_sum / (double)vc;
    a.f.io.d_info[tree * 4 + 0] = max_depth;
    a.f.io.d_info[tree * 4 + 1] = flags;
    a.f.io.d_info[tree * 4 + 2] = tape_pos;
    a.f.io.d_info[tree * 4 + 3] = sum_depth;
  }
  if (a.f.export_trees) {  // parity / diagnose export: LDS records -> the arena's TreeLayout
    TreeRef t;
    t.base = a.f.export_trees + (size_t)tree * a.f.L.tree_bytes;
    t.L = a.f.L;
    for (int n = sub; n < n_nodes; n += FUSED_ROW) {
      const Fc2Node r = nodes[n];
      t.value_sum(n) = r.value_sum; t.reward(n) = r.reward; t.visit(n) = r.visit; t.to_play(n) = r.to_play;
      t.parent(n) = r.parent; t.parent_slot(n) = r.parent_slot;
      for (int s = 0; s < A; ++s) {
        const Fc2Slot q = slots[n * AW + s];
        t.prior(n, s) = q.prior; t.slot_q(n, s) = q.q; t.slot_visit(n, s) = q.n; t.child(n, s) = q.child;
      }
    }
    if (sub == 0) {
      for (int k = 0; k < TM_WORDS; ++k) t.meta(k) = 0;
      t.mm_min() = mm[0]; t.mm_max() = mm[1];
      t.meta(TM_N_NODES) = n_nodes; t.meta(TM_TAPE_POS) = tape_pos; t.meta(TM_FLAGS) = flags;
      t.meta(TM_TIE_DRAWS) = ties; t.meta(TM_MAX_DEPTH) = max_depth; t.meta(TM_SUM_DEPTH) = sum_depth;
      t.meta(TM_ROOT_N) = root_n;
      for (int s = 0; s < A; ++s) t.root_action(s) = roota[s];
    }
    float* hd = a.f.export_hidden + (size_t)tree * NN * E;
    for (int i = sub; i < n_nodes * E; i += FUSED_ROW) hd[i] = hidden[i];
  }
  MZX_PROF(6)
  if (PROFILE && sub == 0 && a.f.prof)
    for (int k = 0; k < FUSED_PROF_WORDS; ++k) a.f.prof[(size_t)tree * FUSED_PROF_WORDS + k] = prof[k];
}

// ---------------------------------------------------------------------------
// host side

struct Fc2Plan {
  Fc2Args args;
  int lds_bytes = 0, ok = 0, small = 0, aw = 0;
};

inline Fc2Plan fc2_plan(const mzx_search* s, bool allow_small = true) {
  Fc2Plan P;
  const FusedPlan base = fused_plan(s, allow_small);   // network recovery + shape limits are shared
  if (!base.ok) return P;
  Fc2Args& a = P.args;
  memset(&a, 0, sizeof(a));
  a.f = base.args;
  P.small = base.small;
  const int A = s->p.num_actions, N = s->p.num_nodes, E = a.f.E;
  const int AW = A <= 2 ? 2 : (A <= 4 ? 4 : 16);
  P.aw = AW;
  auto al16 = [](int64_t x) { return (x + 15) & ~int64_t(15); };
  int64_t o = 0;
  a.f.lds_tables = (int32_t)o;  o += al16(int64_t(16) * (N + 1));
  a.lds_inv = (int32_t)o;       o += al16(int64_t(8) * (N + 2));
  a.f.lds_weights = (int32_t)o; o += P.small ? 0 : al16(int64_t(4) * s->net->num_params);
  a.f.lds_trees = (int32_t)o;
  int64_t t = 0;
  // 2- and 4-lane records: the dead slot row, "node -1", in front of the slots.  It takes the unguarded stores of lanes that
  // own no slot (fc2_backprop, fc2_expand) and is never read: the walk, fc2_load_lane, the export and fc2_from_arena start at
  // node 0.  16-lane records have none (512 bytes a tree: fc2_backprop keeps its guards there).
  t += AW <= 4 ? int64_t(32) * AW : 0;
  a.off_slots = (int32_t)t;   t += int64_t(32) * N * AW;
  a.off_nodes = (int32_t)t;   t += int64_t(32) * N;
  a.off_path = (int32_t)t;    t += al16(int64_t(8) * (N + 1));
  a.off_roota = (int32_t)t;   t += al16(int64_t(4) * AW);
  a.off_mm = (int32_t)t;      t += 16;
  // SmallNet stores a hidden state by the whole row: the lanes >= E spill into the next node's state (written before it is
  // read) or, for node N - 1, into a dead tail of FUSED_ROW - E floats
  a.off_hidden = (int32_t)t;  t += al16(int64_t(4) * (N * E + (P.small && E < FUSED_ROW ? FUSED_ROW - E : 0)));
  a.off_scratch = (int32_t)t; t += int64_t(4) * (P.small ? 16 : FUSED_SCRATCH);
  // the four rows of a wave touch the same offsets of four consecutive slabs in one instruction:
  // keep the slab stride off the multiples of 256 bytes so that they land in different bank groups
  // (bank = (address / 4) mod 64): a stride of 64 (mod 256) bytes puts the rows' records into four different
  // bank groups; with 0 or 128 (mod 256) two rows collide on every access (measured: 43 % of the LDS cycles
  // were bank conflicts at a stride of 128 mod 256, profiles/r02_rocprof_fc2_c2_v1.txt)
  t = al16(t);
  t += (64 - t % 256 + 256) % 256;
  a.tree_stride = (int32_t)t;
  int tpb = 16;
  while (tpb >= 4 && o + int64_t(tpb) * a.tree_stride > FUSED_LDS_BUDGET) tpb /= 2;
  if (tpb < 4) return P;
  a.f.trees_per_block = tpb;
  a.f.tree_stride = a.tree_stride;
  P.lds_bytes = (int)(o + int64_t(tpb) * a.tree_stride);
  P.ok = 1;
  return P;
}

template <class Net, int AW, bool PROFILE, bool CONT = false>
inline int fc2_launch(const Fc2Plan& P, unsigned grid, stream_t stream) {
  static std::atomic<uint64_t> lds_attr_done{0};   // per instantiation, one bit per device
  if (const int ae = allow_large_lds((const void*)fc2_search_kernel<Net, AW, PROFILE, CONT>, FUSED_LDS_BUDGET, lds_attr_done)) {
    set_error("hipFuncSetAttribute: %s", runtime_error_string(ae));
    return MZX_ERR_RUNTIME;
  }
  hipLaunchKernelGGL((fc2_search_kernel<Net, AW, PROFILE, CONT>), dim3(grid), dim3(P.args.f.trees_per_block * FUSED_ROW),
                     (size_t)P.lds_bytes, stream, P.args);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("fused kernel launch failed: %s", hipGetErrorString(e)); return MZX_ERR_RUNTIME; }
  return MZX_OK;
}

template <class Net, bool PROFILE, bool CONT = false>
inline int fc2_launch_aw(const Fc2Plan& P, unsigned grid, stream_t stream) {
  if (P.aw == 2) return fc2_launch<Net, 2, PROFILE, CONT>(P, grid, stream);
  if (P.aw == 4) return fc2_launch<Net, 4, PROFILE, CONT>(P, grid, stream);
  return fc2_launch<Net, 16, PROFILE, CONT>(P, grid, stream);
}

// Whether fc2_search_kernel takes the searches of this handle at its node capacity (num_nodes: num_simulations + 1, or
// what mzx_search_set_capacity set): the per-tree slabs, the pb_c / sqrt tables and the reciprocal table are all sized by
// it.  A capacity whose smallest workgroup (four trees) exceeds FUSED_LDS_BUDGET leaves the handle on the per-operator path.
inline bool fc2_fits(const mzx_search* s) { return fc2_plan(s, !(s->mode & 4)).ok != 0; }

// mode bits: 1 = fused, 2 = export trees to the arena, 4 = force LdsNet, 8 = cycle-profile build
// Handles with spare node capacity (mzx_search_set_capacity) always export, hidden states included: mzx_search_advance
// carries the trees from there.  OVERRIDE: the given roots go in as launch arguments instead of initial_inference.
// CONTINUED: the arena holds carried trees ContinueRootOp prepared; the kernel imports them (CONT instantiation) and writes
// the grown trees back (no profile build).
inline int fc2_run(mzx_search* s, const mzx_search_io* io, void* d_arena, stream_t stream, const SearchStart& start) {
  Fc2Plan P = fc2_plan(s, !(s->mode & 4));
  if (!P.ok) { set_error("fused search kernel does not support this configuration"); return MZX_ERR_INVALID; }
  int rc = ensure_tables(s);
  if (rc) return rc;
  const bool continued = start.kind == SearchStart::CONTINUED;
  if (start.kind == SearchStart::OVERRIDE) {
    P.args.ov_hidden = start.ov.hidden; P.args.ov_priors = start.ov.priors; P.args.ov_reward = start.ov.reward;
  }
  P.args.f.flat = s->net->d_flat;
  P.args.f.tables = s->d_tables;
  P.args.f.io = *io;
  const bool profile = !continued && (s->mode & 8) != 0 && s->ws_floats * 4 >= int64_t(s->p.num_trees) * FUSED_PROF_WORDS * 4;
  if ((s->mode & 2) || s->max_nodes > 0 || continued) {
    P.args.f.export_trees = (char*)d_arena + s->off_trees;
    P.args.f.export_hidden = (float*)((char*)d_arena + s->off_hidden);
  }
  if (profile) P.args.f.prof = (uint32_t*)((char*)d_arena + s->off_ws);
  const int tpb = P.args.f.trees_per_block;
  const unsigned grid = (unsigned)((s->p.num_trees + tpb - 1) / tpb);
  if (continued)
    return P.small ? fc2_launch<SmallNetCartpole, 2, false, true>(P, grid, stream) : fc2_launch_aw<LdsNet, false, true>(P, grid, stream);
  if (P.small)   // SmallNetCartpole has A = 2
    return profile ? fc2_launch<SmallNetCartpole, 2, true>(P, grid, stream)
                   : fc2_launch<SmallNetCartpole, 2, false>(P, grid, stream);
  return profile ? fc2_launch_aw<LdsNet, true>(P, grid, stream) : fc2_launch_aw<LdsNet, false>(P, grid, stream);
}

#endif  // !MZX_HOSTCHECK

}  // namespace mzx
