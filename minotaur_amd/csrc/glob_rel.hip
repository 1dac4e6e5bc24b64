// Glob's relstronger for rounds of any width (mgpu_glob_brancher 1: always
// one node; 2: up to batch nodes), gfx950: StrongBrancher with
// reliabilitySetup(20, 50, 5) (Glob.cpp:171-181; StrongBrancher.cpp) on every
// node of a glob round at once.
//
// The reference runs PCBProcessor::process node by node: the pseudocosts
// change after every node solve (updateAfterSolve, StrongBrancher.cpp:589-643)
// and after every strong-branched candidate (useStrongBranchInfo_, :652-689),
// and a node's solution enters the pool before the next node is processed.
// A round of nb nodes follows this rule (the glob counterpart of the one at
// the top of bnb_rel.hip):
//   * selection: the order-2 pop of mgpu_glob_round (heap top, lazy pruning by
//     the incumbent, up to batch nodes); "node order" is this pop order;
//   * every node sees the round-start incumbent (lazy prune, maxchange =
//     inc - objval, K2's cutoff, the linear presolve's has_inc / inc_ub, the
//     guided dive), the round-start best_x and the round-start pseudocosts,
//     plus the observations it made itself earlier in its own processing
//     (its updateAfterSolve observation and the updatePCost_ pairs of its own
//     strong-branched candidates), applied in the order made;
//   * per node exactly PCBProcessor::process's loop (:214-300): solve, prune,
//     updateAfterSolve on the first pass, feasible, at the root tightenBounds_
//     (root OBBT, glob_obbt_node0 of glob_runtime.cpp; rs_obbt), separate,
//     findBranches, re-solving after OBBT, a cut or a brancher modification;
//   * at the end of the round, node by node in node order, the host folds the
//     node's observation log into the shared pseudocosts (updatePCost_'s
//     running mean, in the order made), takes its incumbent candidate when
//     strictly better, counts its decision and creates its children.
// With one node selected this is the reference's own sequence: kind 1 is this
// code with the round's width fixed at 1, and the root's round of kind 2 is
// always one node wide.
//
// The host (glob_rs_lockstep, glob_runtime.cpp) moves all nodes of the round
// through that loop in lockstep; a node's place in it is RsNode::phase:
//
//   kRsDecided --(dec 1 / 2 / 3 / 4)--------------------------> kRsDone
//       |  --(tangent cuts added)--> kRsSep --LP, decide--> kRsDecided
//       |  --(no candidate: dec 5)----------------------------> kRsDone
//       v  rs_prepare (in rs_post)
//   kRsChild (cand, down) --presolve, LP--> (cand, up) --presolve, LP-->
//       useStrongBranchInfo_: both pruned (dec 1) -------------> kRsDone
//                             one pruned --> kRsMod --presolve (infeasible:
//                                 dec 1 -> kRsDone), LP, decide--> kRsDecided
//                             else the next candidate, or rs_finish (dec 0)
//
// Kernels (one step = rs_child, the batched presolve, rs_masks, up to four LP
// calls, rs_absorb, then for re-solved nodes glob_decide, rs_sdec,
// glob_separate, rs_post; rs_counts closes the step):
//   rs_init    the round's first LP into the per-node state;
//   rs_obbt    the root after root OBBT tightened it: re-solved without a
//              separation pass, or its candidates rebuilt by glob_decide;
//   rs_sdec    glob_separate's view of the decisions (only the nodes just
//              decided);
//   rs_post    after a decision: updateAfterSolve on the first pass, the
//              separation verdict, then rs_prepare (candidate table from
//              glob_decide's io.cand, the reliability split on the node-local
//              counts, reliable scores, vio / minscore, the children's basis)
//              and, with no unreliable candidate to strong-branch, rs_finish;
//   rs_child   Handler::getBrMod of the candidate under way (or of the
//              one-sided verdict) on the node's box and record, into the
//              gathered presolve inputs;
//   rs_masks   the LP skip masks; the separated nodes' own box and record as
//              LP input;
//   rs_absorb  the step's LP results: the child's (status, value), the engine
//              basis, useStrongBranchInfo_, pick, the cursor, rs_finish; a
//              re-solve's result merged for glob_decide;
//   rs_counts  the step's read-back block;
//   rs_children  the branched nodes' children into the pool slots the host
//              assigned in node order.
// One lane per node, as glob_decide: every phase is a short, order-dependent
// sequence (running means, first-maximum scans, the k-th largest vio) over at
// most nv candidates, and bit-equality with the reference needs its
// operation order, which a sequential lane restates directly;
// rs_children alone copies rows and is one wave per node.  A node's data is
// indexed by its position in the round in every array (never compacted), so
// bases, logs and candidate tables of different nodes cannot cross.
// Compiled as glob_tree.hip is (-ffp-contract=off: no fused multiply-add).
#include "glob_internal.h"

namespace mgpu {
namespace {

__device__ __forceinline__ double rs_score(double up, double down) {   // getScore_ (:381-389)
  return up > down ? down * 0.8 + up * 0.2 : up * 0.8 + down * 0.2;
}

__device__ __forceinline__ double rs_keep(double a) { return fabs(a) > 1e-9 ? a : 0.0; }

// StrongBrancher::shouldPrune_ (:461-497)
__device__ __forceinline__ bool rs_prune(double chcutoff, double change, int st, bool *rel) {
  if (st == 3 || st == 2 || st == 5) return true;
  if (st == 1 || st == 0) return change > chcutoff - kSbEps;
  if (st == 6) return false;
  *rel = false;
  return false;
}

// updatePCost_ (:645-650) on the node-local view, and the node's log
__device__ void rs_observe(const RsIO &rs, int b, int nv, int j, double cost, bool down) {
  const size_t o = (size_t)b * nv + j;
  if (down) {
    rs.lpd[o] = (rs.lpd[o] * rs.ltd[o] + cost) / (rs.ltd[o] + 1);
    rs.ltd[o] += 1;
  } else {
    rs.lpu[o] = (rs.lpu[o] * rs.ltu[o] + cost) / (rs.ltu[o] + 1);
    rs.ltu[o] += 1;
  }
  const int k = atomicAdd(&rs.hdr->nobs, 1);
  if (k < rs.obs_cap) {
    rs.obs[k].node = b;
    rs.obs[k].vd = 2 * j + (down ? 1 : 0);
    rs.obs[k].cost = cost;
  } else if (atomicCAS(&rs.hdr->err, 0, 2) == 0) {
    rs.hdr->err_node = b;
  }
}

__device__ void rs_log(const RsIO &rs, int b, int st, int it, double val) {
  RsLog &l = rs.log[b];
  l.flag = 1;
  l.status = st;
  l.iters = it;
  l.value = val;
}

__device__ void rs_copy_basis(const GlobIO &io, int b, int32_t *dh, int8_t *ds, const int32_t *sh,
                              const int8_t *ss) {
  const size_t ho = (size_t)b * io.m, so = (size_t)b * io.N;
  for (int k = 0; k < io.m; ++k) dh[ho + k] = sh[ho + k];
  for (int k = 0; k < io.N; ++k) ds[so + k] = ss[so + k];
}

__device__ __forceinline__ void rs_pick(RsNode &n, int var, double sc, double chu, double chd) {
  if (sc > n.best) {
    n.best = sc;
    n.bc = var;
    n.bdir = chu > chd ? 0 : 1;
  }
}

// the end of findBestCandidate_ (:149-180) and the branching: the pseudocost
// pass over the unreliable candidates not strong-branched, the fallback to
// the first largest violation, the candidate's direction
__device__ void rs_finish(const GlobIO &io, const RsIO &rs, int b, RsNode &n) {
  const int nv = io.nv;
  const size_t o = (size_t)b * nv;
  for (int j = 0; j < nv; ++j) {
    if (rs.ck[o + j] != 2) continue;
    if (rs.cvio[o + j] < n.minscore || j >= n.iend) {
      const double chd = rs.cdd[o + j] * rs.lpd[o + j], chu = rs.cud[o + j] * rs.lpu[o + j];
      rs_pick(n, j, rs_score(chu, chd), chu, chd);
    }
  }
  if (n.best == 0 && n.nrel == 0) {
    int f = -1;
    double top = 0.0;
    for (int j = 0; j < nv; ++j)
      if (rs.ck[o + j] == 2 && (f < 0 || rs.cvio[o + j] > top)) {
        f = j;
        top = rs.cvio[o + j];
      }
    if (f != n.bc) n.bdir = -1;   // setDir was not called for it: UpBranch
    n.bc = f;
  }
  n.phase = kRsDone;
  if (n.bc < 0) {
    n.dec = 5;
    return;
  }
  n.dec = 0;
  n.o_var = n.bc;
  n.o_isint = rs.ci[o + n.bc];
  n.o_dir = n.bdir;
  n.o_v = io.x[o + n.bc];
  n.o_dd = rs.cdd[o + n.bc];
  n.o_ud = rs.cud[o + n.bc];
}

// the candidate loop's cursor (:115-145): the next unreliable candidate at or
// after variable `from` with vio >= minscore, up to maxCands_; none: finish
__device__ void rs_advance(const GlobIO &io, const RsIO &rs, int b, RsNode &n, int from) {
  const int nv = io.nv;
  const size_t o = (size_t)b * nv;
  for (int j = from; j < nv; ++j) {
    if (rs.ck[o + j] != 2) continue;
    if (n.cnt >= kSbCands) {
      n.iend = j;
      rs_finish(io, rs, b, n);
      return;
    }
    if (!(rs.cvio[o + j] >= n.minscore)) continue;
    n.cnt += 1;
    n.cur = j;
    n.side = 0;
    n.phase = kRsChild;
    return;
  }
  n.iend = nv;
  rs_finish(io, rs, b, n);
}

// StrongBrancher::findBranches up to the first strong-branching child
// (:184-264, findBestCandidate_ :93-114, sortUnrelCands_ :429-459)
__device__ void rs_prepare(const GlobIO &io, const RsIO &rs, int b, RsNode &n) {
  const int nv = io.nv;
  const size_t o = (size_t)b * nv;
  // the children's warm start: the engine's basis now (PCBProcessor.cpp:282)
  n.ch_ok = n.has_basis;
  if (n.has_basis) rs_copy_basis(io, b, rs.ch_head, rs.ch_st, rs.cb_head, rs.cb_st);
  const double *id = io.cand + o * 4, *iu = id + nv, *qd = iu + nv, *qu = qd + nv;
  int ncand = 0, nrel = 0, nun = 0;
  n.objval = io.obj[b];
  n.maxchange = rs.inc - n.objval;
  n.best = -INFINITY;
  n.bc = -1;
  n.bdir = -1;
  n.status = 0;
  n.cnt = 0;
  for (int j = 0; j < nv; ++j) {
    const bool hi = id[j] >= 0.0, hq = qd[j] >= 0.0;
    rs.ck[o + j] = 0;
    if (!hi && !hq) continue;
    int isint;
    double d, u;
    if (hi && hq) {
      isint = (id[j] + iu[j] <= qd[j] + qu[j]) ? 0 : 1;
      d = id[j];
      u = iu[j];
    } else if (hi) {
      isint = 1;
      d = id[j];
      u = iu[j];
    } else {
      isint = 0;
      d = qd[j];
      u = qu[j];
    }
    ++ncand;
    rs.ci[o + j] = (int8_t)isint;
    rs.cdd[o + j] = d;
    rs.cud[o + j] = u;
    const int tu = rs.ltu[o + j], td = rs.ltd[o + j];
    if (tu >= kSbThresh && td >= kSbThresh) {
      rs.ck[o + j] = 1;
      ++nrel;
      const double chd = d * rs.lpd[o + j], chu = u * rs.lpu[o + j];
      rs_pick(n, j, rs_score(chu, chd), chu, chd);
    } else {
      rs.ck[o + j] = 2;
      ++nun;
      rs.cvio[o + j] = rs_score(u, d) / (double)((td > tu ? td : tu) + 1);
    }
  }
  n.nrel = nrel;
  if (ncand == 0) {
    n.dec = 5;
    n.phase = kRsDone;
    return;
  }
  // the smallest of the top maxCands_ violations
  n.minscore = 0.0;
  if (nun > 0) {
    const int k = nun < kSbCands ? nun : kSbCands;
    for (int j = 0; j < nv; ++j) {
      if (rs.ck[o + j] != 2) continue;
      const double v = rs.cvio[o + j];
      int g = 0, ge = 0;
      for (int t = 0; t < nv; ++t) {
        if (rs.ck[o + t] != 2) continue;
        g += rs.cvio[o + t] > v ? 1 : 0;
        ge += rs.cvio[o + t] >= v ? 1 : 0;
      }
      if (g < k && k <= ge) {
        n.minscore = v;
        break;
      }
    }
  }
  rs_advance(io, rs, b, n, 0);
}

// Handler::getBrMod of candidate (j, isint) in one direction on the box
// lb / ub and the row state rec, in place: IntVarHandler floor / ceil of x_j;
// QuadHandler x_j itself plus the rows of x_j's violated terms rebuilt for
// the branch's box (getNewSqLf_, getNewBilLf_; with x_j the bilinear's second
// factor the arguments come swapped, as in the reference)
// (QuadHandler.cpp:616-692, 730-763; IntVarHandler.cpp:113-130)
__device__ void rs_br_mod(const GlobIO &io, double *rec, double *lb, double *ub, const double *x,
                          int j, int isint, bool down) {
  const double v = x[j];
  if (isint) {
    if (down) ub[j] = floor(v);
    else lb[j] = ceil(v);
    return;
  }
  const int nsq = io.nsq;
  for (int k = 0; k < nsq; ++k) {
    if (io.sq[2 * k] != j) continue;
    const double yv = x[io.sq[2 * k + 1]], vio = v * v - yv;
    if (vio > 1e-6 && vio > fabs(yv) * 1e-7) {
      const double lo = down ? lb[j] : v, hi = down ? v : ub[j];
      rec[2 * k + 1] = -hi * lo;
      rec[2 * k] = fabs(hi + lo) > 1e-5 ? rs_keep(-1. * (hi + lo)) : 0.0;
    }
  }
  for (int k = 0; k < io.nbil; ++k) {
    const int X0 = io.bil[3 * k], X1 = io.bil[3 * k + 1], y = io.bil[3 * k + 2];
    if (j != X0 && j != X1) continue;
    const double vio = fabs(x[X0] * x[X1] - x[y]);
    if (!(vio > 1e-5 && vio > fabs(x[y]) * 1e-4)) continue;
    const int a = j == X0 ? X0 : X1, bb = j == X0 ? X1 : X0;
    const double xa = x[a];
    const double lb0 = down ? lb[a] : xa, ub0 = down ? xa : ub[a];
    const double lb1 = lb[bb], ub1 = ub[bb];
    double *r0 = rec + 2 * nsq + 12 * k;
    for (int q = 0; q < 2; ++q) {
      const int t = q == 0 ? (down ? 1 : 0) : (down ? 3 : 2);
      double ca, cb, rhs;   // getNewBilLf_: a's, b's coefficient
      if (t == 0) {
        ca = lb1; cb = lb0; rhs = lb0 * lb1;
      } else if (t == 1) {
        ca = ub1; cb = ub0; rhs = ub0 * ub1;
      } else if (t == 2) {
        ca = -1.0 * ub1; cb = -1.0 * lb0; rhs = -lb0 * ub1;
      } else {
        ca = -1.0 * lb1; cb = -1.0 * ub0; rhs = -ub0 * lb1;
      }
      const double c0 = a == X0 ? ca : cb, c1 = a == X0 ? cb : ca;
      double *r = r0 + 3 * t;
      r[0] = rs_keep(c0);
      r[1] = rs_keep(c1);
      r[2] = rhs;
    }
  }
  if (down) ub[j] = v;
  else lb[j] = v;
}

// the node's box and record := the round's LP inputs of the node
__device__ void rs_take_box(const GlobIO &io, const RsIO &rs, int b) {
  const int nv = io.nv, RT = io.R + io.T;
  for (int k = 0; k < nv; ++k) {
    rs.nlb[(size_t)b * nv + k] = io.wlb[(size_t)b * nv + k];
    rs.nub[(size_t)b * nv + k] = io.wub[(size_t)b * nv + k];
  }
  for (int k = 0; k < RT; ++k) rs.nrec[(size_t)b * RT + k] = io.wvals[(size_t)b * RT + k];
}

// the round's first LP (the existing batched presolve, LP and decide ran):
// its log entry, the engine's basis, the node-local pseudocost view
__global__ __launch_bounds__(256) void rs_init(GlobIO io, RsIO rs) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= io.nb) return;
  RsNode &n = rs.node[b];
  const int nv = io.nv;
  for (int j = 0; j < nv; ++j) {
    rs.lpu[(size_t)b * nv + j] = rs.spu[j];
    rs.lpd[(size_t)b * nv + j] = rs.spd[j];
    rs.ltu[(size_t)b * nv + j] = rs.stu[j];
    rs.ltd[(size_t)b * nv + j] = rs.std_[j];
  }
  rs.log[b].flag = 0;
  rs.only[b] = 0;
  if (io.kinf[b] != 0) {   // the presolve closed the node: no LP
    n.dec = io.kinf[b] == 1 ? 1 : 4;
    n.phase = kRsDone;
    return;
  }
  const int st = io.status[b];
  n.lps = 1;
  n.pivots = io.iters[b];
  n.last_val = io.obj[b];
  rs_log(rs, b, st, io.iters[b], io.obj[b]);
  if (st == 0 || st == 6) {
    n.has_basis = 1;
    rs_copy_basis(io, b, rs.cb_head, rs.cb_st, io.wo_head, io.wo_st);
  } else if (io.gok[b] != 0) {
    n.has_basis = 1;
    rs_copy_basis(io, b, rs.cb_head, rs.cb_st, io.ghead, io.gst);
  }
  n.pass = 1;
  n.phase = kRsDecided;
}

// The root (position 0 of its one-node round) after root OBBT wrote a
// tightened box and record into the round's LP inputs (PCBProcessor.cpp:
// 256-280).  resolve: its point left the tightened relaxation, so it is
// solved again there before any separation -- kRsSep without the counted
// re-solve; else glob_decide rebuilds its candidates for the new box.
__global__ void rs_obbt(GlobIO io, RsIO rs, int resolve) {
  if (resolve) {
    rs_take_box(io, rs, 0);
    rs.node[0].phase = kRsSep;
  } else {
    rs.only[0] = 1;
  }
}

__global__ __launch_bounds__(256) void rs_sdec(GlobIO io, RsIO rs) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= io.nb) return;
  rs.sdec[b] = rs.node[b].phase == kRsDecided ? io.dec[b] : 1;
}

// PCBProcessor::process after a solve (:214-300): the decision, the first
// pass's updateAfterSolve, the separation verdict, then findBranches
__global__ __launch_bounds__(256) void rs_post(GlobIO io, RsIO rs) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= io.nb) return;
  RsNode &n = rs.node[b];
  if (n.phase != kRsDecided) return;
  const int d = io.dec[b], nv = io.nv;
  if (d == 1 || d == 2 || d == 4) {
    n.dec = d;
    n.phase = kRsDone;
    return;
  }
  const double obj = io.obj[b];
  if (n.pass == 1 && n.b_var >= 0) {   // StrongBrancher::updateAfterSolve (:589-643)
    const int j = n.b_var;
    const double xj = io.x[(size_t)b * nv + j];
    double cost;
    bool down;
    if (n.b_isint) {
      cost = (obj - n.b_plb) / (fabs(xj - n.b_act) + kSbEps);
      down = xj < n.b_act;
    } else {
      down = n.b_act < 0;
      cost = (obj - n.b_plb) / ((down ? n.b_dd : n.b_ud) + kSbEps);
    }
    if (cost < 0.0 || isinf(cost) || isnan(cost)) cost = 0.0;
    rs_observe(rs, b, nv, j, cost, down);
  }
  if (d == 3) {
    n.dec = 3;
    n.phase = kRsDone;
    return;
  }
  rs_take_box(io, rs, b);   // (with the tangents glob_separate just added)
  if (io.T > 0 && io.flag[b] != 0) {
    n.resolves += 1;
    n.phase = kRsSep;
    return;
  }
  rs_prepare(io, rs, b, n);
}

// the step's read-back block; one block
__global__ __launch_bounds__(256) void rs_counts(GlobIO io, RsIO rs) {
  __shared__ int s_c[4];
  if (threadIdx.x < 4) s_c[threadIdx.x] = 0;
  __syncthreads();
  for (int b = threadIdx.x; b < io.nb; b += 256) {
    const RsNode &n = rs.node[b];
    if (n.phase == kRsChild) atomicAdd(&s_c[0], 1);
    if (n.phase == kRsMod) atomicAdd(&s_c[1], 1);
    if (n.phase == kRsSep) atomicAdd(&s_c[2], 1);
    if ((n.phase == kRsChild || n.phase == kRsMod || n.phase == kRsSep) && !n.has_basis)
      atomicAdd(&s_c[3], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    rs.hdr->n_child = s_c[0];
    rs.hdr->n_mod = s_c[1];
    rs.hdr->n_sep = s_c[2];
    rs.hdr->n_cold = s_c[3];
    rs.hdr->cuts = io.acc[0];
    rs.hdr->flagged = io.acc[1];
  }
}

// the presolve inputs of the step: the node's box and record with the
// candidate's (or the verdict's) getBrMod
__global__ __launch_bounds__(256) void rs_child(GlobIO io, RsIO rs) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= io.nb) return;
  const RsNode &n = rs.node[b];
  rs.log[b].flag = 0;
  if (n.phase != kRsChild && n.phase != kRsMod) return;
  const int nv = io.nv, R = io.R, T = io.T, RT = R + T;
  double *lb = io.glb + (size_t)b * nv, *ub = io.gub + (size_t)b * nv;
  double *rows = io.grows + (size_t)b * R;
  for (int k = 0; k < nv; ++k) {
    lb[k] = rs.nlb[(size_t)b * nv + k];
    ub[k] = rs.nub[(size_t)b * nv + k];
  }
  for (int k = 0; k < R; ++k) rows[k] = rs.nrec[(size_t)b * RT + k];
  for (int k = 0; k < T; ++k) io.gtan[(size_t)b * T + k] = rs.nrec[(size_t)b * RT + R + k];
  const bool down = n.phase == kRsChild ? n.side == 0 : n.mdown != 0;
  rs_br_mod(io, rows, lb, ub, io.x + (size_t)b * nv, n.cur, rs.ci[(size_t)b * nv + n.cur], down);
}

// after the presolve: which LP call solves the node (0 child warm, 1 child
// cold, 2 re-solve warm, 3 re-solve cold); a separated node's own box and
// record (with its new tangents) are its LP input
__global__ __launch_bounds__(256) void rs_masks(GlobIO io, RsIO rs) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= io.nb) return;
  const RsNode &n = rs.node[b];
  const int nb = io.nb, nv = io.nv, RT = io.R + io.T;
  int call = -1;
  if (n.phase == kRsSep) {
    for (int k = 0; k < nv; ++k) {
      const_cast<double *>(io.wlb)[(size_t)b * nv + k] = rs.nlb[(size_t)b * nv + k];
      const_cast<double *>(io.wub)[(size_t)b * nv + k] = rs.nub[(size_t)b * nv + k];
    }
    for (int k = 0; k < RT; ++k) io.wvals[(size_t)b * RT + k] = rs.nrec[(size_t)b * RT + k];
    const_cast<int32_t *>(io.kinf)[b] = 0;
    call = 2;
  } else if ((n.phase == kRsChild || n.phase == kRsMod) && io.kinf[b] == 0) {
    call = n.phase == kRsChild ? 0 : 2;
  }
  if (call >= 0 && !n.has_basis) call += 1;
  for (int k = 0; k < 4; ++k) rs.skip[(size_t)k * nb + b] = k == call ? 0 : 1;
}

// the step's LP results
__global__ __launch_bounds__(256) void rs_absorb(GlobIO io, RsIO rs) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= io.nb) return;
  RsNode &n = rs.node[b];
  rs.only[b] = 0;
  if (n.phase != kRsChild && n.phase != kRsMod && n.phase != kRsSep) return;
  const int nb = io.nb, nv = io.nv;
  const int ki = io.kinf[b];
  if (ki > 1) {   // K2's propagation cap / default bound: an engine problem
    if (atomicCAS(&rs.hdr->err, 0, 1) == 0) rs.hdr->err_node = b;
    n.dec = 4;
    n.phase = kRsDone;
    return;
  }
  const int call = (n.phase == kRsChild ? 0 : 2) + (n.has_basis ? 0 : 1);
  int st = 2;
  double ob = n.last_val;
  if (ki == 0) {
    st = rs.lst[(size_t)call * nb + b];
    ob = rs.lobj[(size_t)call * nb + b];
    const int it = rs.lit[(size_t)call * nb + b];
    n.lps += 1;
    n.last_val = ob;
    rs_log(rs, b, st, it, ob);
    if (st == 0 || st == 6) {
      n.has_basis = 1;
      rs_copy_basis(io, b, rs.cb_head, rs.cb_st, io.wo_head, io.wo_st);
    }
    if (n.phase != kRsChild) {   // a re-solve: the node's LP result for glob_decide
      n.pivots += it;
      n.pass += 1;
      io.status[b] = st;
      io.obj[b] = ob;
      io.iters[b] += it;
      for (int k = 0; k < nv; ++k) io.x[(size_t)b * nv + k] = io.x2[(size_t)b * nv + k];
      rs.only[b] = 1;
      n.phase = kRsDecided;
      return;
    }
    n.sb_lps += 1;
  } else if (n.phase == kRsMod) {   // the modified node is infeasible
    n.dec = 1;
    n.phase = kRsDone;
    return;
  }
  // strongBranch_ (:499-587): the side's (status, value); a child the
  // presolve proved infeasible has no LP: (2, the engine's last value)
  n.sres[n.side] = st;
  n.ores[n.side] = ob;
  if (n.side == 0) {
    n.side = 1;
    return;
  }
  const size_t o = (size_t)b * nv;
  const int j = n.cur;
  const double du = n.ores[1] - n.objval, dd0 = n.ores[0] - n.objval;
  double chu = du < 0.0 ? 0.0 : du, chd = dd0 < 0.0 ? 0.0 : dd0;
  // useStrongBranchInfo_ (:652-689)
  bool is_rel = true;
  const bool pdn = rs_prune(n.maxchange, chd, n.sres[0], &is_rel);
  const bool pup = rs_prune(n.maxchange, chu, n.sres[1], &is_rel);
  if (!is_rel) {
    chu = chd = 0.0;
  } else if (pup && pdn) {
    n.status = 1;
  } else if (pup || pdn) {
    n.status = 2;
    n.mdown = pup ? 1 : 0;
  } else {
    rs_observe(rs, b, nv, j, fabs(chd) / (fabs(rs.cdd[o + j]) + kSbEps), true);
    rs_observe(rs, b, nv, j, fabs(chu) / (fabs(rs.cud[o + j]) + kSbEps), false);
  }
  if (n.status == 1) {
    n.dec = 1;
    n.phase = kRsDone;
    return;
  }
  if (n.status == 2) {
    n.phase = kRsMod;
    return;
  }
  rs_pick(n, j, rs_score(chu, chd), chu, chd);
  rs_advance(io, rs, b, n, j + 1);
}

// One wave per branched node: the down and the up child at the pool slots
// the host assigned, each the node's box with the branching bound, its
// record, the basis saved before strong branching, its value as the bound
__global__ __launch_bounds__(256) void rs_children(GlobIO io, RsIO rs) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= io.nb || rs.cs[2 * b] < 0) return;
  const RsNode &n = rs.node[b];
  const int nv = io.nv, R = io.R, T = io.T, RT = R + T, j = n.o_var;
  const double v = n.o_v;
  const bool isint = n.o_isint != 0;
  const double dn = isint ? floor(v) : v, up = isint ? ceil(v) : v;
  for (int c = 0; c < 2; ++c) {
    const size_t s = (size_t)rs.cs[2 * b + c];
    for (int k = lane; k < nv; k += 64) {
      double l = rs.nlb[(size_t)b * nv + k], u = rs.nub[(size_t)b * nv + k];
      if (k == j) {
        if (c == 1) l = up;
        else u = dn;
      }
      io.plb[s * nv + k] = l;
      io.pub[s * nv + k] = u;
    }
    for (int k = lane; k < R; k += 64) io.prows[s * R + k] = rs.nrec[(size_t)b * RT + k];
    for (int k = lane; k < T; k += 64) io.ptan[s * T + k] = rs.nrec[(size_t)b * RT + R + k];
    if (n.ch_ok) {
      for (int k = lane; k < io.m; k += 64)
        io.pws_head[s * io.m + k] = rs.ch_head[(size_t)b * io.m + k];
      for (int k = lane; k < io.N; k += 64) io.pws_st[s * io.N + k] = rs.ch_st[(size_t)b * io.N + k];
    }
    if (lane == 0) {
      io.pws_ok[s] = n.ch_ok ? 1 : 0;
      io.pnlb[s] = n.objval;
      io.pdepth[s] = io.depth_in[b] + 1;
    }
  }
}

template <class K>
hipError_t launch_lane(K kernel, const GlobIO &io, const RsIO &rs, hipStream_t stream) {
  if (io.nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3((io.nb + 255) / 256), dim3(256), 0, stream, io, rs);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_rs_init(const GlobIO &io, const RsIO &rs, hipStream_t stream) {
  return launch_lane(rs_init, io, rs, stream);
}
hipError_t launch_rs_obbt(const GlobIO &io, const RsIO &rs, int resolve, hipStream_t stream) {
  hipLaunchKernelGGL(rs_obbt, dim3(1), dim3(1), 0, stream, io, rs, resolve);
  return hipGetLastError();
}
hipError_t launch_rs_sdec(const GlobIO &io, const RsIO &rs, hipStream_t stream) {
  return launch_lane(rs_sdec, io, rs, stream);
}
hipError_t launch_rs_post(const GlobIO &io, const RsIO &rs, hipStream_t stream) {
  return launch_lane(rs_post, io, rs, stream);
}
hipError_t launch_rs_child(const GlobIO &io, const RsIO &rs, hipStream_t stream) {
  return launch_lane(rs_child, io, rs, stream);
}
hipError_t launch_rs_masks(const GlobIO &io, const RsIO &rs, hipStream_t stream) {
  return launch_lane(rs_masks, io, rs, stream);
}
hipError_t launch_rs_absorb(const GlobIO &io, const RsIO &rs, hipStream_t stream) {
  return launch_lane(rs_absorb, io, rs, stream);
}

hipError_t launch_rs_counts(const GlobIO &io, const RsIO &rs, hipStream_t stream) {
  if (io.nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(rs_counts, dim3(1), dim3(256), 0, stream, io, rs);
  return hipGetLastError();
}

hipError_t launch_rs_children(const GlobIO &io, const RsIO &rs, hipStream_t stream) {
  if (io.nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(rs_children, dim3((io.nb + 3) / 4), dim3(256), 0, stream, io, rs);
  return hipGetLastError();
}

}  // namespace mgpu
