// Batched spatial branch-and-bound over the McCormick relaxation: the node
// loop of the reference's glob solver (Glob::createBab_, src/solvers/
// Glob.cpp:134-220: BranchAndBound + NodeIncRelaxer + PCBProcessor with
// IntVarHandler, LinearHandler, QuadHandler and, brancher=maxvio,
// MaxVioBrancher; BranchAndBound.cpp:424-514) for a QCQP after
// SimpleTransformer: one round pops the top B open nodes of an HBM stack and
// runs, all on the device,
//   lin  (mgpu_glob_config lin 1) LinearHandler::presolveNode: simplePresolve
//        in node mode over the node's relaxation rows (glob_linear);
//   K2   QuadHandler::presolveNode (QuadHandler.cpp:1204-1269): bound
//        propagation over the products and tightenQuad_, then the rewrite of
//        the node's secant / McCormick rows (upSqCon_ / upBilCon_,
//        :3322-3419) from its PARENT's row state (the incremental
//        relaxation: NodeIncRelaxer keeps the parent's rows, :94-175);
//   K3R + K3   the node's own LP with those rows (OsiLPEngine::
//        changeConstraint then solve, OsiLPEngine.cpp:206-243, 571-652),
//        warm-started from the root basis refactored for the node's matrix
//        (m > 64: K3L with the rows in HBM and the refactorisation inside);
//   decide     shouldPrune_, IntVarHandler + QuadHandler isFeasible, and
//        MaxVioBrancher over both handlers' candidates (glob_tree.hip),
//        spatial branching at the LP value on a continuous variable;
//   OBBT (mgpu_glob_config obbt 1, the root only) QuadHandler::
//        postSolveRootNode's bound LPs, chained on a bound-tightening
//        context of its own (bte_), then the root re-solved when its point
//        left the tightened relaxation (PCBProcessor.cpp:256-280);
//   children   two per branched node, each with the node's tightened box,
//        the branching bound and the node's rows.
// One small record comes back per round (counts, best feasible node).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "bnb_internal.h"
#include "ctx.h"
#include "glob_internal.h"
#include "node_heap.h"
#include "quad_state.h"

// The device buffers sized by the round (ensure_glob_batch; every use is
// behind an ensure of its own size) and nothing else: the next tree of the
// same context takes the whole struct over, so a tree at a batch seen before
// allocates nothing inside a round.  Pool-sized and problem-sized buffers
// stay with GlobState.
struct GlobRoundBufs {
  DevBuf wlb, wub, wrows, kinf, knm, st, obj, it, x, cand, dec, bvar, bval, bup, bint, pos,
      depth_in, out;
  DevBuf wvals, flag, skip2, st2, obj2, it2, x2, acc;   // the separation loop
  DevBuf gsel, cslots, glb, gub, grows, gtan, gdepth, ghead, gst, gok, skip_a;
  DevBuf wo_head, wo_st, wo_d, wo_binv;            // the round's optimal bases
  DevBuf flb, fub, finf, fflag;                    // the linear presolve's scratch
  // the lockstep: the per-node device state of glob_rel.hip in one buffer
  // sized by the widest round (rs_carve)
  DevBuf rs_buf;
};

// The pool-side workspaces of a migration exchange (glob_reserve_migration
// sizes them for a pick size S): kept across trees like the round's buffers.
struct GlobMigBufs {
  DevBuf mw_slots, mw_ft, mw_tmp, mw_stage;
};

struct GlobState : GlobRoundBufs, GlobMigBufs {
  int nv = 0, R = 0, S = 0, T = 0, cap = 0, count = 0, maxb = 0;
  // mgpu_glob_config at init: order 0 stack / 2 reference heap (node_heap.h);
  // warm 0 the root basis / 1 the parent's basis; qt 1 tightenQuad_ at every
  // node / 0 at the first presolveNode call only
  int order = 0, warm = 0, qt = 1, lin = 0, obbt = 0;
  mgpu_ctx *bte = nullptr;       // root OBBT's bound-tightening engine (bte_)
  // Glob's relstronger (mgpu_glob_brancher 1, 2): per pool slot the branching
  // that made the node (updateAfterSolve), and the pseudocosts
  int brancher = 0;
  struct BrInfo {
    int var = -1, isint = 0;
    double act = 0.0, dd = 0.0, ud = 0.0, plb = 0.0;
  };
  std::vector<BrInfo> pinfo;
  std::vector<double> pc_up, pc_dn;
  std::vector<long long> tm_up, tm_dn;
  struct LpRec {
    int32_t status, iters;
    double value;
  };
  std::vector<LpRec> lp_log;     // relstronger: every main-engine solve in order
  // the lockstep: the host's staging of a round
  std::vector<RsNode> rs_hnode;
  std::vector<RsObs> rs_hobs;
  std::vector<std::vector<LpRec>> rs_nlog;   // the round's solves per node
  std::vector<std::vector<RsObs>> rs_nobs;   // the round's observations per node
  std::vector<char> rs_blk;
  std::vector<double> rs_hpc;
  std::vector<int32_t> rs_htm, rs_hcs;
  NodeHeap tree;                 // order 2: the open nodes, their ids and pool slots
  // mgpu_glob_pick: the picked nodes in pick order -- order 0 their pool slots
  // (the stack top, still in place), order 2 the nodes themselves, held out of
  // the heap with their slots until the export (or any other call) settles them
  std::vector<int> pick;
  std::vector<NodeHeap::Node> held;
  std::vector<double> mw_hstage;     // the host side of GlobMigIO::stage
  DevBuf pws_head, pws_st, pws_ok;                 // per pool slot: the parent's basis
  double inc = INFINITY;
  bool root_ws = false;
  std::vector<double> best_x;
  mgpu_glob_stats tot{};
  DevBuf plb, pub, prows, pnlb, pdepth, ptan;
  DevBuf ws_head, ws_st, ws_d, ws_binv, r_st, r_obj, r_it;
  DevBuf fvtype, fsq, fbil, flptr, flvar, flval, fqptr, fqv1, fqv2, fqval, fclb, fcub;
  // the linear presolve (lin 1): the relaxation's term table
  int M = 0, nobj = 0, cons_bad = 0;
  std::vector<int32_t> h_rptr, h_tvar, h_tsrc, h_rhsrc, h_oidx;
  std::vector<double> h_tval, h_rlo, h_rhi, h_oval;
  DevBuf lrptr, ltvar, ltsrc, ltrow, lrhsrc, lcptr, lcterm, loidx, ltval, lrlo, lrhi, loval;
  ~GlobState() {
    if (bte) mgpu_destroy(bte);
  }
  // the round-sized buffers and the OBBT engine of the context's last tree
  void adopt(GlobState &old) {
    static_cast<GlobRoundBufs &>(*this) = std::move(old);
    static_cast<GlobMigBufs &>(*this) = std::move(old);
    std::swap(bte, old.bte);
  }
};

void glob_state_free(mgpu_ctx *c) {
  if (!c) return;
  delete c->glob;
  c->glob = nullptr;
}

namespace {

// The lockstep brancher's device arrays (glob_internal.h RsIO) for rounds of
// up to B nodes, carved from one buffer at `base`; *total: the bytes needed.
// The observation log holds 128 entries per node of the widest round: a
// findBranches call makes at most 2 maxCands_ = 40, so only a node that
// re-solves after modifications several times over, in a round where every
// other node does too, could fill it (the round then ends with an error).
RsIO rs_carve(const GlobState &s, int B, int m, int N, uintptr_t base, size_t *total) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const uintptr_t p = base + off;
    off += (bytes + 15) & ~(size_t)15;
    return p;
  };
  const size_t b = (size_t)B, nv = (size_t)s.nv, RT = (size_t)(s.R + s.T > 0 ? s.R + s.T : 1);
  RsIO r{};
  r.obs_cap = B * 128 + 256;
  r.node = (RsNode *)take(b * sizeof(RsNode));
  r.nlb = (double *)take(b * nv * 8);
  r.nub = (double *)take(b * nv * 8);
  r.nrec = (double *)take(b * RT * 8);
  r.ck = (int8_t *)take(b * nv);
  r.ci = (int8_t *)take(b * nv);
  r.cdd = (double *)take(b * nv * 8);
  r.cud = (double *)take(b * nv * 8);
  r.cvio = (double *)take(b * nv * 8);
  r.lpu = (double *)take(b * nv * 8);
  r.lpd = (double *)take(b * nv * 8);
  r.ltu = (int32_t *)take(b * nv * 4);
  r.ltd = (int32_t *)take(b * nv * 4);
  r.spu = (const double *)take(2 * nv * 8);
  r.spd = r.spu + nv;
  r.stu = (const int32_t *)take(2 * nv * 4);
  r.std_ = r.stu + nv;
  r.cb_head = (int32_t *)take(b * (size_t)m * 4);
  r.ch_head = (int32_t *)take(b * (size_t)m * 4);
  r.cb_st = (int8_t *)take(b * (size_t)N);
  r.ch_st = (int8_t *)take(b * (size_t)N);
  r.skip = (int32_t *)take(4 * b * 4);
  r.lst = (int32_t *)take(4 * b * 4);
  r.lit = (int32_t *)take(4 * b * 4);
  r.lobj = (double *)take(4 * b * 8);
  r.only = (int32_t *)take(b * 4);
  r.sdec = (int32_t *)take(b * 4);
  static_assert(sizeof(RsHdr) % 16 == 0, "the log follows the header");
  r.hdr = (RsHdr *)take(sizeof(RsHdr));
  r.log = (RsLog *)take(b * sizeof(RsLog));
  r.obs = (RsObs *)take((size_t)r.obs_cap * sizeof(RsObs));
  *total = off;
  return r;
}

// the nodes of the last mgpu_glob_pick that were not exported are open nodes
// like any other again (order 2: back in the heap under their own ids)
void glob_settle_pick(GlobState &s) {
  for (const NodeHeap::Node &n : s.held) s.tree.put_back(n);
  s.held.clear();
  s.pick.clear();
}

int ensure_glob_batch(mgpu_ctx *c, GlobState &s, int B) {
  if (B <= s.maxb) return MGPU_OK;
  if (s.brancher >= 1) {
    size_t total = 0;
    (void)rs_carve(s, B, c->lp.m, s.nv + c->lp.m, 0, &total);
    HIPCHK(c, s.rs_buf.ensure(total));
    // the host's staging, so that a round of a width seen before allocates
    // nothing on either side
    s.rs_hnode.reserve((size_t)B);
    s.rs_hobs.reserve((size_t)B * 128 + 256);
    s.rs_nlog.resize((size_t)B);
    s.rs_nobs.resize((size_t)B);
    s.rs_blk.reserve(sizeof(RsHdr) + (size_t)B * sizeof(RsLog));
    s.rs_hcs.reserve((size_t)B * 2);
  }
  const size_t nv = (size_t)s.nv, R = (size_t)(s.R > 0 ? s.R : 1);
  HIPCHK(c, s.wlb.ensure((size_t)B * nv * 8));
  HIPCHK(c, s.wub.ensure((size_t)B * nv * 8));
  HIPCHK(c, s.wrows.ensure((size_t)B * R * 8));
  HIPCHK(c, s.x.ensure((size_t)B * nv * 8));
  HIPCHK(c, s.cand.ensure((size_t)B * nv * 4 * 8));
  for (DevBuf *b : {&s.kinf, &s.knm, &s.st, &s.it, &s.dec, &s.bvar, &s.pos, &s.depth_in})
    HIPCHK(c, b->ensure((size_t)B * 4));
  for (DevBuf *b : {&s.obj, &s.bval}) HIPCHK(c, b->ensure((size_t)B * 8));
  for (DevBuf *b : {&s.bup, &s.bint}) HIPCHK(c, b->ensure((size_t)B));
  HIPCHK(c, s.out.ensure(sizeof(GlobOut)));
  if (s.T > 0) HIPCHK(c, s.wvals.ensure((size_t)B * (R + s.T) * 8));
  for (DevBuf *b : {&s.flag, &s.skip2, &s.st2, &s.it2, &s.skip_a}) HIPCHK(c, b->ensure((size_t)B * 4));
  HIPCHK(c, s.obj2.ensure((size_t)B * 8));
  HIPCHK(c, s.x2.ensure((size_t)B * nv * 8));
  HIPCHK(c, s.acc.ensure(16));
  if (s.order == 2) {
    HIPCHK(c, s.gsel.ensure((size_t)B * 4));
    HIPCHK(c, s.cslots.ensure((size_t)B * 2 * 4));
    HIPCHK(c, s.glb.ensure((size_t)B * nv * 8));
    HIPCHK(c, s.gub.ensure((size_t)B * nv * 8));
    HIPCHK(c, s.grows.ensure((size_t)B * R * 8));
    HIPCHK(c, s.gtan.ensure((size_t)B * (s.T > 0 ? s.T : 1) * 8));
    HIPCHK(c, s.gdepth.ensure((size_t)B * 4));
  }
  if (s.warm == 1) {
    const size_t m = (size_t)c->lp.m, N = (size_t)nv + m;
    HIPCHK(c, s.ghead.ensure((size_t)B * m * 4));
    HIPCHK(c, s.gst.ensure((size_t)B * N));
    HIPCHK(c, s.gok.ensure((size_t)B));
    HIPCHK(c, s.wo_head.ensure((size_t)B * m * 4));
    HIPCHK(c, s.wo_st.ensure((size_t)B * N));
    HIPCHK(c, s.wo_d.ensure((size_t)B * N * 8));
    HIPCHK(c, s.wo_binv.ensure((size_t)B * m * m * 8));
  }
  if (s.lin) {
    HIPCHK(c, s.flb.ensure((size_t)B * nv * 8));
    HIPCHK(c, s.fub.ensure((size_t)B * nv * 8));
    HIPCHK(c, s.finf.ensure((size_t)B * 4));
    HIPCHK(c, s.fflag.ensure((size_t)B * (s.M > 0 ? s.M : 1)));
  }
  s.maxb = B;
  return MGPU_OK;
}

// The relaxation's rows as LinearHandler sees them (the rows of
// quad.relaxation_lp, in its order): the linear rows with every product
// replaced by its auxiliary (duplicates summed, |a| <= 1e-9 dropped, terms
// ascending), one secant row per square, four McCormick rows per bilinear,
// S tangent rows per square.  Record offsets: the secant [a_x, rhs] at 2k,
// bilinear k's row t [a0, a1, rhs] at 2 nsq + 12 k + 3 t, tangent slot t of
// square k [2 xl, xl^2] at R + 2 (k S + t).
int build_linear_table(mgpu_ctx *c, GlobState &s) {
  const QuadState &q = *c->quad;
  const int nsq = (int)q.sq_x.size(), nbil = (int)q.bil_x0.size(), R = q.R, S = s.S;
  std::map<std::pair<int, int>, int> aux;
  for (int k = 0; k < nsq; ++k) aux[{q.sq_x[k], q.sq_x[k]}] = q.sq_y[k];
  for (int k = 0; k < nbil; ++k) aux[{q.bil_x0[k], q.bil_x1[k]}] = q.bil_y[k];
  struct T {
    int var, src;
    double val;
  };
  std::vector<int32_t> rptr{0}, tvar, tsrc, trow, rhsrc;
  std::vector<double> tval, rlo, rhi;
  auto add_row = [&](std::vector<T> terms, double lo, double hi, int hsrc) {
    std::sort(terms.begin(), terms.end(), [](const T &a, const T &b) { return a.var < b.var; });
    const int r = (int)rlo.size();
    for (const T &t : terms) {
      tvar.push_back(t.var);
      tsrc.push_back(t.src);
      tval.push_back(t.val);
      trow.push_back(r);
    }
    rptr.push_back((int32_t)tvar.size());
    rlo.push_back(lo);
    rhi.push_back(hi);
    rhsrc.push_back(hsrc);
  };
  auto linearize = [&](int f, std::vector<T> &out) -> int {
    std::map<int, double> d;
    for (int t = q.h_lptr[f]; t < q.h_lptr[f + 1]; ++t) d[q.h_lvar[t]] += q.h_lval[t];
    for (int t = q.h_qptr[f]; t < q.h_qptr[f + 1]; ++t) {
      auto it = aux.find({q.h_qv1[t], q.h_qv2[t]});
      if (it == aux.end()) it = aux.find({q.h_qv2[t], q.h_qv1[t]});
      if (it == aux.end()) return -1;
      d[it->second] += q.h_qval[t];
    }
    for (const auto &e : d)
      if (std::fabs(e.second) > 1e-9) out.push_back({e.first, -1, e.second});
    return 0;
  };
  int bad = 0;
  for (int f = 0; f < q.ncon; ++f) {
    std::vector<T> terms;
    if (linearize(f, terms) != 0)
      return fail(c, MGPU_ERR_ARG, "mgpu_glob_init: a product of function %d has no auxiliary", f);
    add_row(terms, q.h_clb[f], q.h_cub[f], -1);
    if (q.h_clb[f] > q.h_cub[f] + 1e-8) bad = 1;
  }
  for (int k = 0; k < nsq; ++k)
    add_row({{q.sq_x[k], 2 * k, 0.0}, {q.sq_y[k], -1, 1.0}}, -INFINITY, 0.0, 2 * k + 1);
  for (int k = 0; k < nbil; ++k)
    for (int t = 0; t < 4; ++t) {
      const int o = 2 * nsq + 12 * k + 3 * t;
      add_row({{q.bil_x0[k], o, 0.0}, {q.bil_x1[k], o + 1, 0.0},
               {q.bil_y[k], -1, t < 2 ? -1.0 : 1.0}}, -INFINITY, 0.0, o + 2);
    }
  for (int k = 0; k < nsq; ++k)
    for (int t = 0; t < S; ++t) {
      const int o = R + 2 * (k * S + t);
      add_row({{q.sq_x[k], o, 0.0}, {q.sq_y[k], -1, -1.0}}, -INFINITY, 0.0, o + 1);
    }
  std::vector<T> ob;
  if (q.has_obj && linearize(q.ncon, ob) != 0)
    return fail(c, MGPU_ERR_ARG, "mgpu_glob_init: a product of the objective has no auxiliary");
  std::vector<int32_t> oidx;
  std::vector<double> oval;
  for (const T &t : ob) {
    oidx.push_back(t.var);
    oval.push_back(t.val);
  }
  // column incidence (term indices)
  const int nv = s.nv, nt = (int)tvar.size();
  std::vector<int32_t> cptr((size_t)nv + 1, 0), cterm((size_t)nt);
  for (int t = 0; t < nt; ++t) ++cptr[(size_t)tvar[t] + 1];
  for (int j = 0; j < nv; ++j) cptr[(size_t)j + 1] += cptr[(size_t)j];
  std::vector<int32_t> fill(cptr.begin(), cptr.end() - 1);
  for (int t = 0; t < nt; ++t) cterm[(size_t)fill[(size_t)tvar[t]]++] = t;
  s.M = (int)rlo.size();
  s.nobj = (int)oidx.size();
  s.cons_bad = bad;
  s.h_rptr = rptr;
  s.h_tvar = tvar;
  s.h_tsrc = tsrc;
  s.h_tval = tval;
  s.h_rlo = rlo;
  s.h_rhi = rhi;
  s.h_rhsrc = rhsrc;
  s.h_oidx = oidx;
  s.h_oval = oval;
  if (!s.lin) return MGPU_OK;
  HIPCHK(c, upload(s.lrptr, rptr.data(), rptr.size()));
  HIPCHK(c, upload(s.ltvar, tvar.data(), tvar.size()));
  HIPCHK(c, upload(s.ltsrc, tsrc.data(), tsrc.size()));
  HIPCHK(c, upload(s.ltrow, trow.data(), trow.size()));
  HIPCHK(c, upload(s.ltval, tval.data(), tval.size()));
  HIPCHK(c, upload(s.lrlo, rlo.data(), rlo.size()));
  HIPCHK(c, upload(s.lrhi, rhi.data(), rhi.size()));
  HIPCHK(c, upload(s.lrhsrc, rhsrc.data(), rhsrc.size()));
  HIPCHK(c, upload(s.lcptr, cptr.data(), cptr.size()));
  HIPCHK(c, upload(s.lcterm, cterm.data(), cterm.size()));
  HIPCHK(c, upload(s.loidx, oidx.data(), oidx.size()));
  HIPCHK(c, upload(s.loval, oval.data(), oval.size()));
  return MGPU_OK;
}

// ---- root OBBT: QuadHandler::postSolveRootNode (QuadHandler.cpp:1397-1547)
// with tightenLP_ (:2218-2297), on the host around device LPs -- the same
// restatement as minotaur_amd/obbt.py obbt_chained (pinned bit for bit
// against the reference's postSolveRootNode), here inside the glob round.
constexpr double kObbtMaxVio = 1e-3, kObbtGap = 0.01, kObbtBTol = 1e-8, kObbtRTol = 1e-7;

// the itmp marks of postSolveRootNode (:1410-1517): 1 lower, 2 upper, 3 both
void obbt_marks(const QuadState &q, const double *x, const double *lb, const double *ub,
                std::vector<int> &itmp) {
  itmp.assign((size_t)q.nv, 0);
  for (size_t k = 0; k < q.sq_x.size(); ++k) {
    const int y = q.sq_y[k], x0 = q.sq_x[k];
    const double yv = x[y], xv = x[x0];
    double vio1 = std::fabs(xv * xv - yv);
    if (vio1 > kObbtMaxVio && vio1 > 0.1 * std::fabs(yv)) {
      if (ub[x0] - lb[x0] >= 2) itmp[(size_t)x0] = 3;
      if (ub[y] - lb[y] >= 2) {
        vio1 = yv - lb[y];
        itmp[(size_t)y] = (vio1 > kObbtMaxVio && vio1 > 0.1 * lb[y]) ? 3 : 2;
      }
    }
  }
  auto mark = [&](int v) {
    int &t = itmp[(size_t)v];
    if (!(ub[v] - lb[v] >= 2 && t != 3)) return;
    const double vio1 = x[v] - lb[v], vio2 = ub[v] - x[v];
    if (vio1 > kObbtMaxVio && vio1 > 0.1 * std::fabs(lb[v])) {
      if (vio2 > kObbtMaxVio && vio2 > 0.1 * std::fabs(ub[v])) t = 3;
      else t = t == 2 ? 3 : 1;
    } else if (vio2 > kObbtMaxVio && vio2 > std::fabs(ub[v])) {
      t = t == 1 ? 3 : 2;
    }
  };
  for (size_t k = 0; k < q.bil_x0.size(); ++k) {
    const int y = q.bil_y[k], x0 = q.bil_x0[k], x1 = q.bil_x1[k];
    const double yv = x[y];
    const double vio1 = std::fabs(x[x0] * x[x1] - yv);
    if (vio1 > kObbtMaxVio && vio1 > 0.1 * std::fabs(yv)) {
      mark(x0);
      mark(x1);
      mark(y);
    }
  }
}

// setItmpFromSol_ (:2173-2216) with p_'s current bounds
void obbt_itmp_from_sol(std::vector<int> &itmp, const double *xs, const double *lb,
                        const double *ub) {
  for (size_t v = 0; v < itmp.size(); ++v) {
    const int t = itmp[v];
    if (t == 0) continue;
    const double l = lb[v], u = ub[v], xv = xs[v];
    if (t == 1) {
      if ((xv - l) / (u - l) <= kObbtGap) itmp[v] = 0;
    } else if (t == 2) {
      if ((u - xv) / (u - l) <= kObbtGap) itmp[v] = 0;
    } else {
      if ((xv - l) / (u - l) <= kObbtGap) itmp[v] = 2;
      if ((u - xv) / (u - l) <= kObbtGap) itmp[v] = 1;
    }
  }
}

// updatePBounds_ (:3248-3320): -1 infeasible, 1 a bound moved, 0 none
int obbt_update_bounds(int v, double nlb, double nub, int vtype, double *lb, double *ub) {
  if (vtype <= 3) {
    nub = std::floor(nub);
    nlb = std::ceil(nlb);
  }
  const double L = lb[v], U = ub[v];
  if (nlb > U + kObbtBTol || nub < L - kObbtBTol) return -1;
  const bool lo = nlb > L + kObbtBTol && (L == -INFINITY || nlb > L + kObbtRTol * std::fabs(L));
  const bool up = nub < U - kObbtBTol && (U == INFINITY || nub < U - kObbtRTol * std::fabs(U));
  if (lo && up) {
    lb[v] = nlb;
    ub[v] = nub;
    return 1;
  }
  if (lo) {
    lb[v] = nlb;
    return 1;
  }
  if (up) {
    ub[v] = nub;
    return 1;
  }
  return 0;
}

// upSqCon_ / upBilCon_ (:3322-3419) over every square, then every bilinear,
// on the row state rows[R] with the box lb / ub
void obbt_update_rows(const QuadState &q, const double *lb, const double *ub, double *rows) {
  const double eps = 1e-6 / 10.0;
  auto keep = [](double a) { return std::fabs(a) > 1e-9 ? a : 0.0; };
  const int nsq = (int)q.sq_x.size();
  for (int k = 0; k < nsq; ++k) {
    double *r = rows + 2 * k;
    const double l = lb[q.sq_x[k]], u = ub[q.sq_x[k]], ax = r[0];
    if ((l * l + ax * l < r[1] - eps) || (u * u + ax * u < r[1] - eps)) {
      r[1] = -u * l;
      r[0] = std::fabs(u + l) > 1e-5 ? keep(-1. * (u + l)) : 0.0;
    }
  }
  for (size_t k = 0; k < q.bil_x0.size(); ++k) {
    const int x0 = q.bil_x0[k], x1 = q.bil_x1[k];
    const double l0 = lb[x0], u0 = ub[x0], l1 = lb[x1], u1 = ub[x1];
    double *r = rows + 2 * nsq + 12 * k;
    if (r[0] * l0 + r[1] * l1 - l0 * l1 < r[2] - eps || r[0] * l0 + r[1] * u1 - l0 * u1 < r[2] - eps ||
        r[0] * u0 + r[1] * l1 - u0 * l1 < r[2] - eps) {
      r[0] = keep(l1);
      r[1] = keep(l0);
      r[2] = l0 * l1;
    }
    r += 3;
    if (r[0] * l0 + r[1] * u1 - l0 * u1 < r[2] - eps || r[0] * u0 + r[1] * l1 - u0 * l1 < r[2] - eps ||
        r[0] * u0 + r[1] * u1 - u0 * u1 < r[2] - eps) {
      r[0] = keep(u1);
      r[1] = keep(u0);
      r[2] = u0 * u1;
    }
    r += 3;
    if (r[0] * l0 + r[1] * l1 + l0 * l1 < r[2] - eps || r[0] * l0 + r[1] * u1 + l0 * u1 < r[2] - eps ||
        r[0] * u0 + r[1] * u1 + u0 * u1 < r[2] - eps) {
      r[0] = keep(-1.0 * u1);
      r[1] = keep(-1.0 * l0);
      r[2] = -l0 * u1;
    }
    r += 3;
    if (r[0] * l0 + r[1] * l1 + l0 * l1 < r[2] - eps || r[0] * u0 + r[1] * l1 + u0 * l1 < r[2] - eps ||
        r[0] * u0 + r[1] * u1 + u0 * u1 < r[2] - eps) {
      r[0] = keep(-1.0 * l1);
      r[1] = keep(-1.0 * u0);
      r[2] = -u0 * l1;
    }
  }
}

// a row's weight / upper side with the node record rec [R + T]
inline double tab_w(const GlobState &s, const double *rec, int t) {
  return s.h_tsrc[(size_t)t] < 0 ? s.h_tval[(size_t)t] : rec[s.h_tsrc[(size_t)t]];
}
inline double tab_hi(const GlobState &s, const double *rec, int r) {
  return s.h_rhsrc[(size_t)r] < 0 ? s.h_rhi[(size_t)r] : rec[s.h_rhsrc[(size_t)r]];
}

// isFeasibleToRelaxation_ (:955-981): x against every relaxation row
bool obbt_rel_feasible(const GlobState &s, const double *rec, const double *x) {
  for (int r = 0; r < s.M; ++r) {
    double act = 0.0;
    for (int t = s.h_rptr[(size_t)r]; t < s.h_rptr[(size_t)r + 1]; ++t) {
      const double a = tab_w(s, rec, t);
      if (std::fabs(a) > 1e-9) act += a * x[s.h_tvar[(size_t)t]];
    }
    const double cub = tab_hi(s, rec, r), clb = s.h_rlo[(size_t)r];
    if ((act > cub + 1e-6) && (cub == 0 || act > cub + std::fabs(cub) * 1e-7)) return false;
    if ((act < clb - 1e-6) && (clb == 0 || act < clb - std::fabs(clb) * 1e-7)) return false;
  }
  return true;
}

// postSolveRootNode on the root (batch index 0 of the first round): x its LP
// point, lb / ub its box, rec its record; tightens lb / ub / rec in place.
// *changed: a bound moved (rows rewritten); *feasible: x still satisfies
// the tightened relaxation.  *nlps: bound LPs solved.
int glob_root_obbt(mgpu_ctx *c, GlobState &s, const double *x, std::vector<double> &lb,
                   std::vector<double> &ub, std::vector<double> &rec, bool *changed,
                   bool *feasible, long long *nlps) {
  const QuadState &q = *c->quad;
  const int nv = s.nv;
  *changed = false;
  *feasible = true;
  std::vector<int> itmp;
  obbt_marks(q, x, lb.data(), ub.data(), itmp);
  // tightenLP_: the relaxation cloned with the root's bounds and rows (the
  // free rows of unused tangent slots left out: the reference has no such
  // row), plus the objective cutoff row with an incumbent (:2232-2244)
  std::vector<int32_t> rptr{0}, cidx, ctype((size_t)nv);
  std::vector<double> val, rlo, rhi;
  const int R = s.R;
  for (int r = 0; r < s.M; ++r) {
    const double hi = tab_hi(s, rec.data(), r);
    if (s.h_rhsrc[(size_t)r] >= R && hi == INFINITY) continue;
    for (int t = s.h_rptr[(size_t)r]; t < s.h_rptr[(size_t)r + 1]; ++t) {
      const double a = tab_w(s, rec.data(), t);
      if (std::fabs(a) <= 1e-9) continue;
      cidx.push_back(s.h_tvar[(size_t)t]);
      val.push_back(a);
    }
    rptr.push_back((int32_t)cidx.size());
    rlo.push_back(s.h_rlo[(size_t)r]);
    rhi.push_back(hi);
  }
  if (std::isfinite(s.inc) && q.has_obj) {
    for (size_t k = 0; k < s.h_oidx.size(); ++k) {
      cidx.push_back(s.h_oidx[k]);
      val.push_back(s.h_oval[k]);
    }
    rptr.push_back((int32_t)cidx.size());
    rlo.push_back(-INFINITY);
    rhi.push_back(s.inc - q.obj_const);
  }
  for (int j = 0; j < nv; ++j) ctype[(size_t)j] = q.h_vtype[(size_t)j];
  const int m = (int)rlo.size(), N = nv + m;
  const std::vector<double> lb0 = lb, ub0 = ub;   // the clone's bounds stay as loaded
  if (!s.bte) {
    int rc = mgpu_create(c->device, &s.bte);
    if (rc != MGPU_OK) return fail(c, rc, "mgpu_glob_round: the OBBT engine: mgpu_create failed");
    mgpu_set_stream(s.bte, c->stream);
  }
  std::vector<double> obj((size_t)nv, 0.0), xs((size_t)nv), wd((size_t)N), wb((size_t)m * m),
      ib((size_t)m * m);
  std::vector<int32_t> wh((size_t)m), ih((size_t)m);
  std::vector<int8_t> wst((size_t)N), ist((size_t)N);
  bool have_ws = false;   // bte_->load drops the warm start: the first LP from the slack basis
  // getBndByLP_ (:2080-2109): the bound LP min sign x_v from the last
  // optimal basis (HipLPEngine keeps a basis after ProvenOptimal /
  // EngineIterationLimit), its reduced costs rebuilt for the new objective
  auto bound_lp = [&](int v, double sign, double *b, bool *inf) -> int {
    std::fill(obj.begin(), obj.end(), 0.0);
    obj[(size_t)v] = sign;
    int rc = mgpu_load_lp(s.bte, nv, m, rptr.data(), cidx.data(), val.data(), rlo.data(),
                          rhi.data(), lb0.data(), ub0.data(), ctype.data(), obj.data(), 0.0);
    if (rc != MGPU_OK) return fail(c, rc, "mgpu_glob_round: OBBT load: %s", mgpu_last_error(s.bte));
    int32_t st = 0, it = 0;
    double ov = 0.0;
    rc = mgpu_lp_solve(s.bte, 1, lb0.data(), ub0.data(), nullptr, have_ws ? ih.data() : nullptr,
                       have_ws ? ist.data() : nullptr, nullptr, have_ws ? ib.data() : nullptr, 1, 0,
                       &st, &ov, &it, xs.data(), wh.data(), wst.data(), wd.data(), wb.data());
    if (rc != MGPU_OK) return fail(c, rc, "mgpu_glob_round: OBBT solve: %s", mgpu_last_error(s.bte));
    ++*nlps;
    if (st == 0 || st == 6) {
      ih.swap(wh);
      ist.swap(wst);
      ib.swap(wb);
      have_ws = true;
    }
    *inf = !(st == 0 || st == 6 || st == 4);
    *b = *inf ? INFINITY : ov;
    return MGPU_OK;
  };
  for (int v = 0; v < nv; ++v) {
    const int t = itmp[(size_t)v];
    if (t == 0) continue;
    double nlb = -INFINITY, nub = INFINITY, b = 0.0;
    bool inf = false;
    if (t == 1 || t == 3) {
      int rc = bound_lp(v, 1.0, &b, &inf);
      if (rc != MGPU_OK) return rc;
      if (inf) continue;
      nlb = b;
      obbt_itmp_from_sol(itmp, xs.data(), lb.data(), ub.data());
    }
    if (t == 2) {
      int rc = bound_lp(v, -1.0, &b, &inf);
      if (rc != MGPU_OK) return rc;
      if (inf) continue;
      nub = -b;
      obbt_itmp_from_sol(itmp, xs.data(), lb.data(), ub.data());
    }
    const int u = obbt_update_bounds(v, nlb, nub, q.h_vtype[(size_t)v], lb.data(), ub.data());
    if (u < 0) break;   // tightenLP_ returns "infeasible" (only logged, :1519-1524)
    if (u > 0) *changed = true;
  }
  if (*changed) {
    obbt_update_rows(q, lb.data(), ub.data(), rec.data());
    *feasible = obbt_rel_feasible(s, rec.data(), x);
  }
  return MGPU_OK;
}

// tightenBounds_ (PCBProcessor.cpp:256-262) on the root, position 0 of its
// one-node round, after its first solve and decision: when it is neither
// pruned nor feasible (decision 0 or 5), postSolveRootNode on its point, box
// and record; a tightened box, rows and record go back into the round's LP
// inputs (wlb / wub / wrows / wvals).  The bound LPs are counted here.
int glob_obbt_node0(mgpu_ctx *c, GlobState &s, const GlobIO &io, bool *changed, bool *feasible) {
  const int nv = s.nv, R = s.R, RT = R + s.T;
  hipStream_t stream = c->stream;
  auto cp = [stream](void *dst, const void *src, size_t bytes, hipMemcpyKind kind) -> hipError_t {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, stream);
    return e != hipSuccess ? e : hipStreamSynchronize(stream);
  };
  *changed = false;
  *feasible = true;
  int32_t d0 = -1;
  HIPCHK(c, cp(&d0, io.dec, 4, hipMemcpyDeviceToHost));
  if (d0 != 0 && d0 != 5) return MGPU_OK;
  std::vector<double> x((size_t)nv), lb((size_t)nv), ub((size_t)nv), rec((size_t)(RT > 0 ? RT : 1));
  HIPCHK(c, cp(x.data(), io.x, (size_t)nv * 8, hipMemcpyDeviceToHost));
  HIPCHK(c, cp(lb.data(), io.wlb, (size_t)nv * 8, hipMemcpyDeviceToHost));
  HIPCHK(c, cp(ub.data(), io.wub, (size_t)nv * 8, hipMemcpyDeviceToHost));
  if (RT > 0) HIPCHK(c, cp(rec.data(), io.wvals, (size_t)RT * 8, hipMemcpyDeviceToHost));
  int rc = glob_root_obbt(c, s, x.data(), lb, ub, rec, changed, feasible, &s.tot.obbt_lps);
  if (rc != MGPU_OK || !*changed) return rc;
  HIPCHK(c, cp(s.wlb.p, lb.data(), (size_t)nv * 8, hipMemcpyHostToDevice));
  HIPCHK(c, cp(s.wub.p, ub.data(), (size_t)nv * 8, hipMemcpyHostToDevice));
  if (R > 0) HIPCHK(c, cp(s.wrows.p, rec.data(), (size_t)R * 8, hipMemcpyHostToDevice));
  if (s.T > 0) HIPCHK(c, cp(io.wvals, rec.data(), (size_t)RT * 8, hipMemcpyHostToDevice));
  return MGPU_OK;
}

// ---- Glob's relstronger (mgpu_glob_brancher 1: one node per round; 2: up to
// batch nodes) ----------------------------------------------------------------
// The rule is at the top of glob_rel.hip.  The round's first presolve, LP and
// decide ran in mgpu_glob_round; from there every node walks PCBProcessor::
// process's loop, all nodes in lockstep: a step stages the strong-branching
// children and modifications (rs_child), presolves them in one batch, solves
// them (children: iteration limit 50; re-solves: the default) under skip
// masks, and absorbs the results (rs_absorb); nodes re-solved after a
// modification or a tangent cut are decided and separated again (glob_decide,
// glob_separate, rs_post).  One small block comes back per step: the counts
// of nodes by what they wait for and the step's solves for the LP log.  The
// launches always cover all nb positions; what a node does in a step is a
// phase test in the kernels and a skip mask in the LP calls.  The engine's
// basis is one slot per node (rs.cb_*), the output of a solve that ends
// optimal or at the iteration limit becoming the next solve's start, as the
// reference's one engine chains it.  The root's round (always one node) runs
// root OBBT between the root's first decision and its separation.
int glob_rs_lockstep(mgpu_ctx *c, GlobState &s, GlobIO &io,
                     const std::vector<NodeHeap::Node> &popped, mgpu_glob_stats *stats) {
  const int nb = io.nb, nv = s.nv, T = s.T, m = c->lp.m, N = nv + m;
  hipStream_t stream = c->stream;
  size_t total = 0;
  RsIO rs = rs_carve(s, s.maxb, m, N, (uintptr_t)s.rs_buf.p, &total);
  rs.inc = s.inc;
  // the round-start state every node sees
  const double inc0 = s.inc;
  const std::vector<double> bx0 = s.best_x;
  s.rs_hnode.assign((size_t)nb, RsNode{});
  for (int b = 0; b < nb; ++b) {
    const GlobState::BrInfo &bi = s.pinfo[(size_t)popped[(size_t)b].slot];
    RsNode &n = s.rs_hnode[(size_t)b];
    n.b_var = bi.var;
    n.b_isint = bi.isint;
    n.b_act = bi.act;
    n.b_dd = bi.dd;
    n.b_ud = bi.ud;
    n.b_plb = bi.plb;
    s.rs_nlog[(size_t)b].clear();
    s.rs_nobs[(size_t)b].clear();
  }
  s.rs_hpc.resize((size_t)nv * 2);
  s.rs_htm.resize((size_t)nv * 2);
  for (int j = 0; j < nv; ++j) {
    s.rs_hpc[(size_t)j] = s.pc_up[(size_t)j];
    s.rs_hpc[(size_t)(nv + j)] = s.pc_dn[(size_t)j];
    s.rs_htm[(size_t)j] = (int32_t)s.tm_up[(size_t)j];
    s.rs_htm[(size_t)(nv + j)] = (int32_t)s.tm_dn[(size_t)j];
  }
  HIPCHK(c, hipMemcpyAsync(rs.node, s.rs_hnode.data(), (size_t)nb * sizeof(RsNode),
                           hipMemcpyHostToDevice, stream));
  HIPCHK(c, hipMemcpyAsync(const_cast<double *>(rs.spu), s.rs_hpc.data(), (size_t)nv * 16,
                           hipMemcpyHostToDevice, stream));
  HIPCHK(c, hipMemcpyAsync(const_cast<int32_t *>(rs.stu), s.rs_htm.data(), (size_t)nv * 8,
                           hipMemcpyHostToDevice, stream));
  HIPCHK(c, hipMemsetAsync(rs.hdr, 0, sizeof(RsHdr), stream));
  HIPCHK(c, launch_rs_init(io, rs, stream));
  GlobIO sio = io;   // glob_separate: only the nodes just decided
  sio.dec = rs.sdec;
  GlobIO dio = io;   // glob_decide: only the nodes just re-solved
  dio.only = rs.only;
  GlobIO pio = io;   // the presolve of the staged children / modifications
  pio.flb_in = io.glb;
  pio.fub_in = io.gub;
  pio.frows = io.grows;
  pio.ftan = io.gtan;
  pio.in_tan = io.gtan;
  LpWarmOut wo{s.wo_head.as<int32_t>(), s.wo_st.as<int8_t>(), s.wo_d.as<double>(),
               s.wo_binv.as<double>()};
  auto lp = [&](int call, bool warm, int limit) {
    const size_t o = (size_t)call * nb;
    return lp_solve_rows_wo(c, nb, io.wlb, io.wub, rs.skip + o, io.wvals, warm ? rs.cb_head : nullptr,
                            warm ? rs.cb_st : nullptr, warm ? 0 : 1, limit, rs.lst + o, rs.lobj + o,
                            rs.lit + o, s.x2.as<double>(), nullptr, &wo);
  };
  const size_t blk_bytes = sizeof(RsHdr) + (size_t)nb * sizeof(RsLog);
  s.rs_blk.resize(blk_bytes);
  RsHdr hdr{};
  long long cuts = 0;
  bool post = true;
  if (s.obbt && popped[0].id == 0) {   // the root's first pass: tightenBounds_
    bool changed = false, feasible = true;
    int rc = glob_obbt_node0(c, s, io, &changed, &feasible);
    if (rc != MGPU_OK) return rc;
    if (changed) {
      // its point left the tightened relaxation: re-solved there and decided
      // again, no separation in between (SepaResolve); else separation and
      // findBranches on the same point, the candidates from the new box
      HIPCHK(c, launch_rs_obbt(io, rs, feasible ? 0 : 1, stream));
      if (feasible) HIPCHK(c, launch_glob_decide(dio, stream));
      post = feasible;
    }
  }
  // a node strong-branches at most 20 candidates (two steps each) per pass and
  // re-solves after a modification only with a tighter box; far below this
  const long max_steps = 1L << 20;
  for (long step = 0;; ++step) {
    if (post) {
      if (T > 0) {   // separate_: the squares' tangents (glob_separate)
        HIPCHK(c, hipMemsetAsync(s.acc.p, 0, 16, stream));
        HIPCHK(c, launch_rs_sdec(io, rs, stream));
        HIPCHK(c, launch_glob_separate(sio, stream));
      }
      HIPCHK(c, launch_rs_post(io, rs, stream));
    }
    HIPCHK(c, launch_rs_counts(io, rs, stream));
    HIPCHK(c, hipMemcpyAsync(s.rs_blk.data(), rs.hdr, blk_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    std::memcpy(&hdr, s.rs_blk.data(), sizeof hdr);
    const RsLog *lg = reinterpret_cast<const RsLog *>(s.rs_blk.data() + sizeof(RsHdr));
    for (int b = 0; b < nb; ++b)
      if (lg[b].flag) s.rs_nlog[(size_t)b].push_back({lg[b].status, lg[b].iters, lg[b].value});
    if (post && T > 0) cuts += (long long)hdr.cuts;
    if (hdr.err == 1)
      return fail(c, MGPU_ERR_ENGINE, "mgpu_glob_round: K2 failed on a strong-branching child or "
                  "a modification of node %d of the round", hdr.err_node);
    if (hdr.err == 2)
      return fail(c, MGPU_ERR_NOMEM, "mgpu_glob_round: the observation log (%d entries) is full "
                  "at node %d of the round", rs.obs_cap, hdr.err_node);
    if (hdr.n_child + hdr.n_mod + hdr.n_sep == 0) break;
    if (step >= max_steps)
      return fail(c, MGPU_ERR_ENGINE, "mgpu_glob_round: the lockstep did not end in %ld steps",
                  max_steps);
    HIPCHK(c, launch_rs_child(io, rs, stream));
    if (hdr.n_child + hdr.n_mod > 0) {   // the handlers' presolveNode on the staged boxes
      HIPCHK(c, launch_glob_linear(pio, stream));
      int r2 = mgpu_quad_fbbt_dev(c, nb, io.flb, io.fub, s.inc, s.qt, io.grows, 0, s.wlb.as<double>(),
                                  s.wub.as<double>(), s.wrows.as<double>(), s.kinf.as<int32_t>(),
                                  s.knm.as<int32_t>(), 0, nullptr, nullptr, nullptr, nullptr);
      if (r2 != MGPU_OK) return r2;
      HIPCHK(c, launch_glob_linear_verdict(pio, stream));
      if (T > 0) HIPCHK(c, launch_glob_pack(pio, stream));
    }
    HIPCHK(c, launch_rs_masks(io, rs, stream));
    int rc = MGPU_OK;
    if (hdr.n_child > 0) {
      rc = lp(0, true, kSbIter);
      if (rc == MGPU_OK && hdr.n_cold > 0) rc = lp(1, false, kSbIter);
    }
    if (rc == MGPU_OK && hdr.n_mod + hdr.n_sep > 0) {
      rc = lp(2, true, 0);
      if (rc == MGPU_OK && hdr.n_cold > 0) rc = lp(3, false, 0);
    }
    if (rc != MGPU_OK) return rc;
    HIPCHK(c, launch_rs_absorb(io, rs, stream));
    post = hdr.n_mod + hdr.n_sep > 0;
    if (post) HIPCHK(c, launch_glob_decide(dio, stream));
  }
  // ---- the end of the round, node by node in node order ----
  s.rs_hobs.resize((size_t)(hdr.nobs > 0 ? hdr.nobs : 0));
  s.rs_blk.resize((size_t)nb * 8);   // (the nodes' LP values, for the incumbent candidates)
  HIPCHK(c, hipMemcpyAsync(s.rs_hnode.data(), rs.node, (size_t)nb * sizeof(RsNode),
                           hipMemcpyDeviceToHost, stream));
  if (hdr.nobs > 0)
    HIPCHK(c, hipMemcpyAsync(s.rs_hobs.data(), rs.obs, (size_t)hdr.nobs * sizeof(RsObs),
                             hipMemcpyDeviceToHost, stream));
  HIPCHK(c, hipMemcpyAsync(s.rs_blk.data(), io.obj, (size_t)nb * 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(c, hipStreamSynchronize(stream));
  const double *objv = reinterpret_cast<const double *>(s.rs_blk.data());
  for (const RsObs &ob : s.rs_hobs) s.rs_nobs[(size_t)ob.node].push_back(ob);   // (in the order made)
  s.rs_hcs.assign((size_t)nb * 2, -1);
  bool kids = false;
  long long ndec4 = 0;
  for (int b = 0; b < nb; ++b) {
    const RsNode &n = s.rs_hnode[(size_t)b];
    for (const RsObs &ob : s.rs_nobs[(size_t)b]) {   // updatePCost_ (:645-650)
      const size_t j = (size_t)(ob.vd >> 1);
      if (ob.vd & 1) {
        s.pc_dn[j] = (s.pc_dn[j] * s.tm_dn[j] + ob.cost) / (s.tm_dn[j] + 1);
        s.tm_dn[j] += 1;
      } else {
        s.pc_up[j] = (s.pc_up[j] * s.tm_up[j] + ob.cost) / (s.tm_up[j] + 1);
        s.tm_up[j] += 1;
      }
    }
    for (const GlobState::LpRec &r : s.rs_nlog[(size_t)b]) s.lp_log.push_back(r);
    s.tot.ndec[n.dec] += 1;
    s.tot.lps += n.lps;
    s.tot.pivots += n.pivots;
    s.tot.sb_lps += n.sb_lps;
    s.tot.resolves += n.resolves;
    if (n.dec == 4) ++ndec4;
    if (n.dec == 3 && objv[b] < s.inc) {
      s.inc = objv[b];
      HIPCHK(c, hipMemcpy(s.best_x.data(), s.x.as<double>() + (size_t)b * nv, (size_t)nv * 8,
                          hipMemcpyDeviceToHost));
    }
    if (n.dec != 0) continue;
    // the children (QuadHandler::getBranches down, up; IntVarHandler's guided
    // dive on the round-start incumbent, else the candidate's direction)
    const int j = n.o_var;
    const bool isint = n.o_isint != 0;
    const bool df = down_first(isint, n.o_dir != 0, true, inc0, bx0[(size_t)j], n.o_v);
    if (isint) s.tot.br_int += 1;
    else s.tot.br_cont += 1;
    for (int k = 0; k < 2; ++k) {
      const bool upc = df ? k == 1 : k == 0;
      const int slot = s.tree.take_slot();
      s.rs_hcs[(size_t)(2 * b + (upc ? 1 : 0))] = slot;
      GlobState::BrInfo bi;
      bi.var = j;
      bi.isint = n.o_isint;
      bi.act = isint ? n.o_v : (upc ? 1.0 : -1.0);
      bi.dd = n.o_dd;
      bi.ud = n.o_ud;
      bi.plb = n.objval;
      s.pinfo[(size_t)slot] = bi;
      s.tree.push(n.objval, popped[(size_t)b].depth + 1, slot);
      kids = true;
    }
  }
  if (kids) {
    HIPCHK(c, hipMemcpyAsync(s.cslots.p, s.rs_hcs.data(), (size_t)nb * 8, hipMemcpyHostToDevice,
                             stream));
    rs.cs = s.cslots.as<int32_t>();
    HIPCHK(c, launch_rs_children(io, rs, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
  }
  s.count = s.tree.open();
  s.tot.rounds += 1;
  s.tot.nodes += nb;
  s.tot.cuts += cuts;
  s.tot.open = s.count;
  s.tot.last_batch = nb;
  s.tot.incumbent = s.inc;
  if (stats) *stats = s.tot;
  if (ndec4 > 0)
    return fail(c, MGPU_ERR_ENGINE, "mgpu_glob_round: %lld nodes ended with an engine problem "
                "(K2 propagation cap / default bound, or an unbounded / unknown LP status)", ndec4);
  return MGPU_OK;
}

}  // namespace

extern "C" {

int mgpu_glob_brancher(mgpu_ctx *c, int kind) {
  if (!c) return MGPU_ERR_ARG;
  if (kind < 0 || kind > 2)
    return fail(c, MGPU_ERR_ARG, "mgpu_glob_brancher: kind %d (0 MaxVio, 1 relstronger one node "
                "per round, 2 relstronger batched)", kind);
  c->glob_brancher = kind;
  return MGPU_OK;
}

int mgpu_glob_config(mgpu_ctx *c, int order, int warm, int qt, int lin, int obbt) {
  if (!c) return MGPU_ERR_ARG;
  if ((order != 0 && order != 2) || warm < 0 || warm > 1 || qt < 0 || qt > 1 || lin < 0 ||
      lin > 1 || obbt < 0 || obbt > 1)
    return fail(c, MGPU_ERR_ARG, "mgpu_glob_config: order %d (0, 2), warm %d (0, 1), qt %d (0, 1), "
                "lin %d (0, 1), obbt %d (0, 1)", order, warm, qt, lin, obbt);
  c->glob_order = order;
  c->glob_warm = warm;
  c->glob_qt = qt;
  c->glob_lin = lin;
  c->glob_obbt = obbt;
  return MGPU_OK;
}

int mgpu_glob_init(mgpu_ctx *c, int capacity, double incumbent) {
  if (!c) return MGPU_ERR_ARG;
  if (!c->loaded || !c->quad || !c->nr_set)
    return fail(c, MGPU_ERR_STATE, "mgpu_glob_init: load the relaxation LP (mgpu_load_lp), the "
                "quadratic problem (mgpu_load_quad) and the node-rows map first");
  const QuadState &q = *c->quad;
  const int nsq = (int)q.sq_x.size();
  // record = R row-state values, then 2 S tangent values per square
  const int extra = c->nr_stride - q.R;
  if (c->lp.n != q.nv || extra < 0 || (extra > 0 && (nsq == 0 || extra % (2 * nsq) != 0)))
    return fail(c, MGPU_ERR_ARG, "mgpu_glob_init: LP columns (%d) / row-record stride (%d) do "
                "not match the quadratic problem (%d vars, %d row values, %d squares)", c->lp.n,
                c->nr_stride, q.nv, q.R, nsq);
  if (capacity < 1) return fail(c, MGPU_ERR_ARG, "mgpu_glob_init: capacity < 1");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  GlobState *s = new GlobState();
  if (c->glob) s->adopt(*c->glob);
  glob_state_free(c);
  c->glob = s;
  const int nv = q.nv, R = q.R, m = c->lp.m, N = nv + m;
  s->nv = nv;
  s->R = R;
  s->order = c->glob_order;
  s->warm = c->glob_warm;
  s->qt = c->glob_qt;
  s->lin = c->glob_lin;
  s->obbt = c->glob_obbt;
  s->brancher = c->glob_brancher;
  if (s->brancher >= 1 && (s->order != 2 || s->warm != 1 || s->lin != 1))
    return fail(c, MGPU_ERR_ARG, "mgpu_glob_init: relstronger needs order 2, warm 1 and lin 1 "
                "(a brancher's modification reaches p_ only through LinearHandler's "
                "copyBndsFromRel_)");
  if (s->brancher >= 1) {
    s->pinfo.assign((size_t)capacity, GlobState::BrInfo{});
    s->pc_up.assign((size_t)nv, 0.0);
    s->pc_dn.assign((size_t)nv, 0.0);
    s->tm_up.assign((size_t)nv, 0);
    s->tm_dn.assign((size_t)nv, 0);
  }
  s->T = extra;
  s->S = nsq > 0 ? extra / (2 * nsq) : 0;
  if (s->lin || s->obbt) {
    const int rc0 = build_linear_table(c, *s);
    if (rc0 != MGPU_OK) return rc0;
  }
  s->cap = capacity;
  s->inc = incumbent;
  s->best_x.assign((size_t)nv, NAN);
  s->tot.incumbent = incumbent;
  HIPCHK(c, s->plb.ensure((size_t)capacity * nv * 8));
  HIPCHK(c, s->pub.ensure((size_t)capacity * nv * 8));
  HIPCHK(c, s->prows.ensure((size_t)capacity * (R > 0 ? R : 1) * 8));
  HIPCHK(c, s->pnlb.ensure((size_t)capacity * 8));
  HIPCHK(c, s->pdepth.ensure((size_t)capacity * 4));
  // the problem data of the decision kernel
  std::vector<uint8_t> vt((size_t)nv);
  for (int j = 0; j < nv; ++j) vt[(size_t)j] = (uint8_t)q.h_vtype[(size_t)j];
  HIPCHK(c, upload(s->fvtype, vt.data(), vt.size()));
  HIPCHK(c, upload(s->flptr, q.h_lptr.data(), q.h_lptr.size()));
  HIPCHK(c, upload(s->flvar, q.h_lvar.data(), q.h_lvar.size()));
  HIPCHK(c, upload(s->flval, q.h_lval.data(), q.h_lval.size()));
  HIPCHK(c, upload(s->fqptr, q.h_qptr.data(), q.h_qptr.size()));
  HIPCHK(c, upload(s->fqv1, q.h_qv1.data(), q.h_qv1.size()));
  HIPCHK(c, upload(s->fqv2, q.h_qv2.data(), q.h_qv2.size()));
  HIPCHK(c, upload(s->fqval, q.h_qval.data(), q.h_qval.size()));
  HIPCHK(c, upload(s->fclb, q.h_clb.data(), q.h_clb.size()));
  HIPCHK(c, upload(s->fcub, q.h_cub.data(), q.h_cub.size()));
  // the root: the loaded column bounds, QuadHandler::relax_'s rows there
  std::vector<double> lb((size_t)nv), ub((size_t)nv), rows((size_t)(R > 0 ? R : 1));
  HIPCHK(c, hipMemcpy(lb.data(), c->collb.p, (size_t)nv * 8, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(ub.data(), c->colub.p, (size_t)nv * 8, hipMemcpyDeviceToHost));
  int rc = mgpu_quad_rows(c, lb.data(), ub.data(), rows.data(), nullptr);
  if (rc != MGPU_OK) return rc;
  const double ninf = -INFINITY;
  const int32_t zero = 0;
  HIPCHK(c, hipMemcpy(s->plb.p, lb.data(), (size_t)nv * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(s->pub.p, ub.data(), (size_t)nv * 8, hipMemcpyHostToDevice));
  if (R > 0) HIPCHK(c, hipMemcpy(s->prows.p, rows.data(), (size_t)R * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(s->pnlb.p, &ninf, 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(s->pdepth.p, &zero, 4, hipMemcpyHostToDevice));
  if (s->T > 0) {   // the root's tangent slots, all free: [0, +inf]
    HIPCHK(c, s->ptan.ensure((size_t)capacity * s->T * 8));
    std::vector<double> t0((size_t)s->T, 0.0);
    for (int k = 1; k < s->T; k += 2) t0[(size_t)k] = INFINITY;
    HIPCHK(c, hipMemcpy(s->ptan.p, t0.data(), (size_t)s->T * 8, hipMemcpyHostToDevice));
  }
  s->count = 1;
  if (s->order == 2) {   // the root is node 0 in slot 0
    s->tree.reset(capacity);
  }
  if (s->warm == 1) {    // per slot: the parent's basis; the root has none (slack basis)
    HIPCHK(c, s->pws_head.ensure((size_t)capacity * m * 4));
    HIPCHK(c, s->pws_st.ensure((size_t)capacity * N));
    HIPCHK(c, s->pws_ok.ensure((size_t)capacity));
    HIPCHK(c, hipMemset(s->pws_ok.p, 0, (size_t)capacity));
  }
  // the root basis every node LP refactors for its own rows: the loaded LP
  // (the root's rows) from the slack basis
  HIPCHK(c, s->ws_head.ensure((size_t)m * 4 + 4));
  HIPCHK(c, s->ws_st.ensure((size_t)N));
  HIPCHK(c, s->ws_d.ensure((size_t)N * 8));
  HIPCHK(c, s->ws_binv.ensure((size_t)m * m * 8 + 8));
  for (DevBuf *b : {&s->r_st, &s->r_it}) HIPCHK(c, b->ensure(4));
  HIPCHK(c, s->r_obj.ensure(8));
  rc = mgpu_lp_solve_dev(c, 1, c->collb.as<double>(), c->colub.as<double>(), nullptr, nullptr,
                         nullptr, nullptr, nullptr, 1, 0, s->r_st.as<int32_t>(),
                         s->r_obj.as<double>(), s->r_it.as<int32_t>(), nullptr,
                         s->ws_head.as<int32_t>(), s->ws_st.as<int8_t>(), s->ws_d.as<double>(),
                         s->ws_binv.as<double>());
  if (rc != MGPU_OK) return rc;
  int32_t rst = 0;
  HIPCHK(c, hipMemcpyAsync(&rst, s->r_st.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  s->root_ws = rst == 0;
  s->tot.open = 1;
  return MGPU_OK;
}

int mgpu_glob_round(mgpu_ctx *c, int batch, double incumbent, mgpu_glob_stats *stats) {
  if (!c) return MGPU_ERR_ARG;
  if (!c->glob) return fail(c, MGPU_ERR_STATE, "mgpu_glob_round: mgpu_glob_init first");
  if (batch < 1) return fail(c, MGPU_ERR_ARG, "mgpu_glob_round: batch < 1");
  GlobState &s = *c->glob;
  glob_settle_pick(s);
  if (s.brancher == 1) batch = 1;   // relstronger: the reference's node at a time
  const QuadState &q = *c->quad;
  HIPCHK(c, hipSetDevice(c->device));
  if (incumbent < s.inc) {  // an outside incumbent: no point of ours matches it
    s.inc = incumbent;
    std::fill(s.best_x.begin(), s.best_x.end(), NAN);
  }
  const bool heap = s.order == 2;
  const int nv = s.nv, R = s.R, m = c->lp.m, N = nv + m;
  int nb = 0, base = 0;
  std::vector<int32_t> sel;
  NodeHeap::Round round;
  if (heap) {
    round = s.tree.take(batch, s.inc);
    for (const NodeHeap::Node &nd : round.nodes) sel.push_back(nd.slot);
    nb = (int)sel.size();
    if (!round.fits)
      return fail(c, MGPU_ERR_NOMEM, "mgpu_glob_round: node pool full (%d slots)", s.cap);
  } else {
    nb = batch < s.count ? batch : s.count;
    if (s.count + nb > s.cap) nb = s.cap - s.count;  // children must fit: base + 2 nb <= cap
    if (nb <= 0 && s.count > 0) return fail(c, MGPU_ERR_NOMEM, "mgpu_glob_round: node pool full");
    base = s.count - nb;
  }
  if (nb <= 0) {
    s.count = heap ? 0 : s.count;
    s.tot.open = 0;
    if (stats) *stats = s.tot;
    return MGPU_OK;
  }
  int rc = ensure_glob_batch(c, s, nb);
  if (rc != MGPU_OK) return rc;
  GlobIO io{};
  io.nb = nb;
  io.base = base;
  io.nv = nv;
  io.R = R;
  io.m = m;
  io.N = N;
  io.vtype = s.fvtype.as<uint8_t>();
  io.nsq = (int)q.sq_x.size();
  io.nbil = (int)q.bil_x0.size();
  io.ncon = q.ncon;
  io.nfun = q.ncon + (q.has_obj ? 1 : 0);
  io.sq = q.dq.sq;
  io.bil = q.dq.bil;
  io.lptr = s.flptr.as<int32_t>();
  io.lvar = s.flvar.as<int32_t>();
  io.lval = s.flval.as<double>();
  io.qptr = s.fqptr.as<int32_t>();
  io.qv1 = s.fqv1.as<int32_t>();
  io.qv2 = s.fqv2.as<int32_t>();
  io.qval = s.fqval.as<double>();
  io.clb = s.fclb.as<double>();
  io.cub = s.fcub.as<double>();
  io.obj_const = q.obj_const;
  io.inc = s.inc;
  io.abs_tol = 1e-6;   // solAbs_tol / solRel_tol (Environment.cpp:486, 509-528)
  io.rel_tol = 1e-6;
  io.kinf = s.kinf.as<int32_t>();
  io.wlb = s.wlb.as<double>();
  io.wub = s.wub.as<double>();
  io.wrows = s.wrows.as<double>();
  io.status = s.st.as<int32_t>();
  io.iters = s.it.as<int32_t>();
  io.obj = s.obj.as<double>();
  io.x = s.x.as<double>();
  io.cand = s.cand.as<double>();
  io.dec = s.dec.as<int32_t>();
  io.bvar = s.bvar.as<int32_t>();
  io.pos = s.pos.as<int32_t>();
  io.depth_in = s.depth_in.as<int32_t>();
  io.bval = s.bval.as<double>();
  io.bup = s.bup.as<int8_t>();
  io.bint = s.bint.as<int8_t>();
  io.out = s.out.as<GlobOut>();
  io.plb = s.plb.as<double>();
  io.pub = s.pub.as<double>();
  io.prows = s.prows.as<double>();
  io.pnlb = s.pnlb.as<double>();
  io.pdepth = s.pdepth.as<int32_t>();
  io.S = s.S;
  io.T = s.T;
  io.ptan = s.T > 0 ? s.ptan.as<double>() : nullptr;
  io.wvals = s.T > 0 ? s.wvals.as<double>() : s.wrows.as<double>();
  io.flag = s.flag.as<int32_t>();
  io.skip2 = s.skip2.as<int32_t>();
  io.skip_a = s.skip_a.as<int32_t>();
  io.st2 = s.st2.as<int32_t>();
  io.it2 = s.it2.as<int32_t>();
  io.obj2 = s.obj2.as<double>();
  io.x2 = s.x2.as<double>();
  io.acc = s.acc.as<unsigned long long>();
  if (s.warm == 1) {
    io.pws_head = s.pws_head.as<int32_t>();
    io.pws_st = s.pws_st.as<int8_t>();
    io.pws_ok = s.pws_ok.as<uint8_t>();
    io.ghead = s.ghead.as<int32_t>();
    io.gst = s.gst.as<int8_t>();
    io.gok = s.gok.as<uint8_t>();
    io.wo_head = s.wo_head.as<int32_t>();
    io.wo_st = s.wo_st.as<int8_t>();
  }
  // the round's input nodes
  const double *in_lb, *in_ub, *in_rows;
  if (heap) {
    HIPCHK(c, hipMemcpyAsync(s.gsel.p, sel.data(), (size_t)nb * 4, hipMemcpyHostToDevice,
                             c->stream));
    io.sel = s.gsel.as<int32_t>();
    io.glb = s.glb.as<double>();
    io.gub = s.gub.as<double>();
    io.grows = s.grows.as<double>();
    io.gtan = s.gtan.as<double>();
    io.gdepth = s.gdepth.as<int32_t>();
    HIPCHK(c, launch_glob_gather(io, c->stream));
    in_lb = io.glb;
    in_ub = io.gub;
    in_rows = io.grows;
    io.in_depth = io.gdepth;
    io.in_tan = io.gtan;
  } else {
    if (s.warm == 1) {   // the stack's top nb slots: their bases in place
      io.ghead = s.pws_head.as<int32_t>() + (size_t)base * m;
      io.gst = s.pws_st.as<int8_t>() + (size_t)base * N;
      io.gok = s.pws_ok.as<uint8_t>() + base;
    }
    in_lb = s.plb.as<double>() + (size_t)base * nv;
    in_ub = s.pub.as<double>() + (size_t)base * nv;
    in_rows = s.prows.as<double>() + (size_t)base * R;
    io.in_depth = s.pdepth.as<int32_t>() + base;
    io.in_tan = s.T > 0 ? s.ptan.as<double>() + (size_t)base * s.T : nullptr;
  }
  // the handlers' presolveNode in order (PCBProcessor.cpp:148-167):
  // LinearHandler's over the node's relaxation rows as the node inherited
  // them, then QuadHandler's on the box that leaves
  if (s.lin) {
    io.M = s.M;
    io.nobj = s.nobj;
    io.cons_bad = s.cons_bad;
    // a solution in the pool (LinearHandler.cpp:1636-1640)
    io.has_inc = std::isfinite(s.inc) ? 1 : 0;
    io.inc_ub = s.inc - q.obj_const;
    io.lrptr = s.lrptr.as<int32_t>();
    io.ltvar = s.ltvar.as<int32_t>();
    io.ltsrc = s.ltsrc.as<int32_t>();
    io.ltrow = s.ltrow.as<int32_t>();
    io.lrhsrc = s.lrhsrc.as<int32_t>();
    io.lcptr = s.lcptr.as<int32_t>();
    io.lcterm = s.lcterm.as<int32_t>();
    io.loidx = s.loidx.as<int32_t>();
    io.ltval = s.ltval.as<double>();
    io.lrlo = s.lrlo.as<double>();
    io.lrhi = s.lrhi.as<double>();
    io.loval = s.loval.as<double>();
    io.flb_in = in_lb;
    io.fub_in = in_ub;
    io.frows = in_rows;
    io.ftan = io.in_tan;
    io.flb = s.flb.as<double>();
    io.fub = s.fub.as<double>();
    io.finf = s.finf.as<int32_t>();
    io.fflag = s.fflag.as<uint8_t>();
    HIPCHK(c, launch_glob_linear(io, c->stream));
    in_lb = io.flb;
    in_ub = io.fub;
  }
  // K2 from the parents' rows; tightenQuad_ at every node (doQT_, set by
  // Glob's presolve) or only at the first presolveNode call (QuadHandler.cpp:
  // 1215, 1241: niters <= 1)
  const int qt = (s.qt || s.tot.nodes == 0) ? 1 : 0;
  rc = mgpu_quad_fbbt_dev(c, nb, in_lb, in_ub, s.inc, qt, in_rows, 0, s.wlb.as<double>(),
                          s.wub.as<double>(), s.wrows.as<double>(), s.kinf.as<int32_t>(),
                          s.knm.as<int32_t>(), 0, nullptr, nullptr, nullptr, nullptr);
  if (rc != MGPU_OK) return rc;
  if (s.lin) HIPCHK(c, launch_glob_linear_verdict(io, c->stream));
  // the node records: K2's rows and the node's tangent slots
  if (s.T > 0) HIPCHK(c, launch_glob_pack(io, c->stream));
  // the node LPs with their own rows (K3R + K3), K2-infeasible nodes skipped.
  // warm 0: every node from the root basis refactored for its rows; warm 1:
  // from its parent's optimal basis refactored for its rows, as HipLPEngine
  // refactors the kept basis after NodeIncRelaxer replays the rows
  // (HipLPEngine::refactor_; OsiLPEngine: Clp), the root from the slack basis
  LpWarmOut wo{s.wo_head.as<int32_t>(), s.wo_st.as<int8_t>(), s.wo_d.as<double>(),
               s.wo_binv.as<double>()};
  auto solve = [&](const int32_t *skip, const int32_t *head, const int8_t *st_in, int shared,
                   const double *binv, int32_t *st, double *obj, int32_t *it, double *x) {
    return lp_solve_rows_wo(c, nb, s.wlb.as<double>(), s.wub.as<double>(), skip, io.wvals, head,
                            st_in, shared, 0, st, obj, it, x, binv,
                            s.warm == 1 ? &wo : nullptr);
  };
  if (s.warm == 1) {
    HIPCHK(c, launch_glob_skips(io, c->stream));
    rc = solve(io.skip_a, io.ghead, io.gst, 0, nullptr, s.st.as<int32_t>(), s.obj.as<double>(),
               s.it.as<int32_t>(), s.x.as<double>());
    if (rc != MGPU_OK) return rc;
    // the nodes without a basis (the root): from the slack basis, into the
    // same x and bases, merged by flag
    bool cold = !heap;
    if (heap)
      for (const NodeHeap::Node &g : round.nodes) cold |= g.id == 0;
    if (cold) {
      rc = solve(io.skip2, nullptr, nullptr, 1, nullptr, s.st2.as<int32_t>(), s.obj2.as<double>(),
                 s.it2.as<int32_t>(), s.x.as<double>());
      if (rc != MGPU_OK) return rc;
      GlobIO mio = io;
      mio.x2 = io.x;   // (the cold call wrote x in place)
      HIPCHK(c, launch_glob_merge(mio, c->stream));
    }
  } else {
    rc = solve(s.kinf.as<int32_t>(), s.root_ws ? s.ws_head.as<int32_t>() : nullptr,
               s.root_ws ? s.ws_st.as<int8_t>() : nullptr, 1,
               s.root_ws ? s.ws_binv.as<double>() : nullptr, s.st.as<int32_t>(),
               s.obj.as<double>(), s.it.as<int32_t>(), s.x.as<double>());
    if (rc != MGPU_OK) return rc;
  }
  HIPCHK(c, launch_glob_decide(io, c->stream));
  // relstronger: the round's nodes through PCBProcessor::process's loop in
  // lockstep (kind 1: batch is 1, the reference's node at a time)
  if (s.brancher >= 1) return glob_rs_lockstep(c, s, io, round.nodes, stats);
  // the flagged nodes (flag / skip2) re-solved -- from the root basis (warm
  // 0) or the node's last basis refactored for its rows (warm 1) -- merged
  // back and decided again
  auto resolve_flagged = [&]() -> int {
    int r;
    if (s.warm == 1)
      r = solve(io.skip2, s.wo_head.as<int32_t>(), s.wo_st.as<int8_t>(), 0, nullptr,
                s.st2.as<int32_t>(), s.obj2.as<double>(), s.it2.as<int32_t>(), s.x2.as<double>());
    else
      r = solve(io.skip2, s.root_ws ? s.ws_head.as<int32_t>() : nullptr,
                s.root_ws ? s.ws_st.as<int8_t>() : nullptr, 1,
                s.root_ws ? s.ws_binv.as<double>() : nullptr, s.st2.as<int32_t>(),
                s.obj2.as<double>(), s.it2.as<int32_t>(), s.x2.as<double>());
    if (r != MGPU_OK) return r;
    HIPCHK(c, launch_glob_merge(io, c->stream));
    GlobIO again = io;
    again.only = io.flag;
    HIPCHK(c, launch_glob_decide(again, c->stream));
    return MGPU_OK;
  };
  // root OBBT (PCBProcessor::process, :256-280): at the root's first solve,
  // when it is neither pruned nor feasible, QuadHandler::postSolveRootNode;
  // if its point leaves the tightened relaxation the root is re-solved
  // (SepaResolve, no separation in between), else it is decided again on the
  // same point with the tightened box
  long long obbt_resolves = 0;
  if (s.obbt && s.tot.nodes == 0 && nb == 1) {
    bool changed = false, feasible = true;
    rc = glob_obbt_node0(c, s, io, &changed, &feasible);
    if (rc != MGPU_OK) return rc;
    if (changed) {
      const int32_t one = 1, zero = 0;
      HIPCHK(c, hipMemcpy(io.flag, &one, 4, hipMemcpyHostToDevice));
      HIPCHK(c, hipMemcpy(io.skip2, &zero, 4, hipMemcpyHostToDevice));
      if (!feasible) {
        rc = resolve_flagged();
        if (rc != MGPU_OK) return rc;
        obbt_resolves = 1;
      } else {
        GlobIO again = io;
        again.only = io.flag;
        HIPCHK(c, launch_glob_decide(again, c->stream));
      }
    }
  }
  // the separation loop (PCBProcessor.cpp:267-280): every pass adds at least
  // one cut to a free slot, so it ends within nsq S passes
  long long cuts = 0, resolves = 0;
  for (int pass = 0; s.T > 0 && pass <= s.T / 2; ++pass) {
    HIPCHK(c, hipMemsetAsync(s.acc.p, 0, 16, c->stream));
    HIPCHK(c, launch_glob_separate(io, c->stream));
    unsigned long long a[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(a, s.acc.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (a[1] == 0) break;
    cuts += (long long)a[0];
    resolves += (long long)a[1];
    rc = resolve_flagged();
    if (rc != MGPU_OK) return rc;
  }
  HIPCHK(c, launch_glob_summary(io, c->stream));
  GlobOut o;
  if (heap) {
    // the children in the reference's branch order (down_first)
    std::vector<int32_t> dec(nb), bvar(nb), pos(nb), dep(nb);
    std::vector<double> obj(nb), bval(nb);
    std::vector<int8_t> bup(nb), bint(nb);
    HIPCHK(c, hipMemcpyAsync(&o, s.out.p, sizeof o, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dec.data(), io.dec, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(bvar.data(), io.bvar, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(pos.data(), io.pos, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dep.data(), io.depth_in, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(obj.data(), io.obj, (size_t)nb * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(bval.data(), io.bval, (size_t)nb * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(bup.data(), io.bup, (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(bint.data(), io.bint, (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the incumbent this round found (for the guided dive of its own nodes'
    // children the reference already has it: a node's solution enters the
    // pool before the next node branches; at batch 1 no other node shares
    // the round)
    std::vector<int32_t> cs((size_t)o.nchild);
    for (int i = 0; i < nb; ++i) {
      if (dec[i] != 0) continue;
      const int s_down = s.tree.take_slot(), s_up = s.tree.take_slot();
      cs[(size_t)pos[i]] = s_down;
      cs[(size_t)pos[i] + 1] = s_up;
      const bool df = down_first(bint[i] != 0, bup[i] != 0, true, s.inc,
                                 s.best_x[(size_t)bvar[i]], bval[i]);
      s.tree.push(obj[i], dep[i] + 1, df ? s_down : s_up);
      s.tree.push(obj[i], dep[i] + 1, df ? s_up : s_down);
    }
    if (!cs.empty()) {
      HIPCHK(c, hipMemcpyAsync(s.cslots.p, cs.data(), cs.size() * 4, hipMemcpyHostToDevice,
                               c->stream));
      io.child_slots = s.cslots.as<int32_t>();
      HIPCHK(c, launch_glob_children(io, c->stream));
    }
    s.count = s.tree.open();
  } else {
    HIPCHK(c, launch_glob_children(io, c->stream));
    HIPCHK(c, hipMemcpyAsync(&o, s.out.p, sizeof o, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.count = base + o.nchild;
  }
  if (o.best_idx >= 0 && o.best < s.inc) {
    s.inc = o.best;
    HIPCHK(c, hipMemcpy(s.best_x.data(), s.x.as<double>() + (size_t)o.best_idx * nv,
                        (size_t)nv * 8, hipMemcpyDeviceToHost));
  }
  s.tot.rounds += 1;
  s.tot.nodes += nb;
  for (int k = 0; k < 6; ++k) s.tot.ndec[k] += o.ndec[k];
  s.tot.lps += o.lps + resolves + obbt_resolves;
  s.tot.pivots += o.pivots;
  s.tot.cuts += cuts;
  s.tot.resolves += resolves;
  s.tot.br_int += o.br_int;
  s.tot.br_cont += o.ndec[0] - o.br_int;
  s.tot.open = s.count;
  s.tot.last_batch = nb;
  s.tot.incumbent = s.inc;
  if (stats) *stats = s.tot;
  if (o.ndec[4] > 0)
    return fail(c, MGPU_ERR_ENGINE, "mgpu_glob_round: %lld nodes ended with an engine problem "
                "(K2 propagation cap / default bound, or an unbounded / unknown LP status)",
                (long long)o.ndec[4]);
  return MGPU_OK;
}

int mgpu_glob_lp_log(mgpu_ctx *c, int cap, int32_t *status, double *value, int32_t *iters) {
  if (!c) return MGPU_ERR_ARG;
  if (!c->glob) return fail(c, MGPU_ERR_STATE, "mgpu_glob_lp_log: mgpu_glob_init first");
  const auto &lg = c->glob->lp_log;
  for (size_t k = 0; k < lg.size() && (int)k < cap; ++k) {
    if (status) status[k] = lg[k].status;
    if (value) value[k] = lg[k].value;
    if (iters) iters[k] = lg[k].iters;
  }
  return (int)lg.size();
}

int mgpu_glob_best(mgpu_ctx *c, double *obj, double *x) {
  if (!c) return MGPU_ERR_ARG;
  if (!c->glob) return fail(c, MGPU_ERR_STATE, "mgpu_glob_best: mgpu_glob_init first");
  if (obj) *obj = c->glob->inc;
  if (x) std::memcpy(x, c->glob->best_x.data(), (size_t)c->glob->nv * 8);
  return MGPU_OK;
}

// Node migration for the node-sharded spatial tree (MpiBranchAndBound::
// LoadBalance_, MpiBranchAndBound.cpp:78-195; the candidates come from
// TreeManager::getCandidate).  mgpu_glob_pick is the pop (the nodes stay open,
// only their bounds leave), mgpu_glob_export_dev packs the chosen ones into
// device rows and removes them, mgpu_glob_import_dev places received rows.
// The row (glob_migrate.hip; mgpu_glob_row_width) carries everything a node's
// processing reads: box, row state, tangent slots, bound, depth, the parent's
// basis (warm 1) and the branching record (relstronger).
}  // extern "C"

namespace {

// every per-slot device array of the pool
std::vector<std::pair<DevBuf *, size_t>> glob_slot_rows(GlobState &s, int m) {
  const size_t nv = (size_t)s.nv, N = nv + (size_t)m;
  std::vector<std::pair<DevBuf *, size_t>> r = {{&s.plb, nv * 8}, {&s.pub, nv * 8},
                                                {&s.prows, (size_t)s.R * 8}, {&s.pnlb, 8},
                                                {&s.pdepth, 4}};
  if (s.T > 0) r.push_back({&s.ptan, (size_t)s.T * 8});
  if (s.warm == 1) {
    r.push_back({&s.pws_head, (size_t)m * 4});
    r.push_back({&s.pws_st, N});
    r.push_back({&s.pws_ok, 1});
  }
  return r;
}

size_t glob_width(const mgpu_ctx *c, const GlobState &s) {
  return glob_mig_width(s.nv, s.R, s.T, c->lp.m, s.warm == 1, s.brancher >= 1);
}

int glob_open(const GlobState &s) {
  return s.order == 2 ? s.tree.open() + (int)s.held.size() : s.count;
}

// the device slot list and the kernels' view of the pool for k rows
int glob_mig_io(mgpu_ctx *c, GlobState &s, const std::vector<int32_t> &slots, double *rows,
                GlobMigIO *io) {
  const int k = (int)slots.size();
  HIPCHK(c, s.mw_slots.ensure((size_t)k * 4));
  HIPCHK(c, s.mw_stage.ensure((size_t)k * kMigStage * 8));
  HIPCHK(c, hipMemcpyAsync(s.mw_slots.p, slots.data(), (size_t)k * 4, hipMemcpyHostToDevice,
                           c->stream));
  *io = GlobMigIO{};
  io->k = k;
  io->nv = s.nv;
  io->R = s.R;
  io->T = s.T;
  io->m = c->lp.m;
  io->N = s.nv + c->lp.m;
  io->W = (int)glob_width(c, s);
  io->warm = s.warm == 1;
  io->br = s.brancher >= 1;
  io->slots = s.mw_slots.as<int32_t>();
  io->rows = rows;
  io->plb = s.plb.as<double>();
  io->pub = s.pub.as<double>();
  io->prows = s.prows.as<double>();
  io->ptan = s.T > 0 ? s.ptan.as<double>() : nullptr;
  io->pnlb = s.pnlb.as<double>();
  io->pdepth = s.pdepth.as<int32_t>();
  if (s.warm == 1) {
    io->pws_head = s.pws_head.as<int32_t>();
    io->pws_st = s.pws_st.as<int8_t>();
    io->pws_ok = s.pws_ok.as<uint8_t>();
  }
  io->stage = s.mw_stage.as<double>();
  return MGPU_OK;
}

// packs the nodes at pool slots `slots` into `buf` (device rows); depth-first:
// the slots lie in the stack's top `region` slots, the others of that region
// keep their order and close the gaps, in every per-slot array
int glob_take_nodes(mgpu_ctx *c, GlobState &s, const std::vector<int32_t> &slots, int region,
                    double *buf) {
  const int k = (int)slots.size();
  if (k == 0) return MGPU_OK;
  GlobMigIO io;
  int rc = glob_mig_io(c, s, slots, buf, &io);
  if (rc != MGPU_OK) return rc;
  if (s.brancher >= 1) {   // the branching records: one staged copy
    s.mw_hstage.assign((size_t)k * kMigStage, 0.0);
    for (int t = 0; t < k; ++t) {
      const GlobState::BrInfo &bi = s.pinfo[(size_t)slots[(size_t)t]];
      double *h = s.mw_hstage.data() + (size_t)t * kMigStage;
      h[2] = (double)bi.var;
      h[3] = (double)bi.isint;
      h[4] = bi.act;
      h[5] = bi.dd;
      h[6] = bi.ud;
      h[7] = bi.plb;
    }
    HIPCHK(c, hipMemcpyAsync(s.mw_stage.p, s.mw_hstage.data(), (size_t)k * kMigStage * 8,
                             hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, launch_glob_mig_pack(io, c->stream));
  if (s.order == 0) {
    const int base = s.count - region;
    std::vector<uint8_t> gone((size_t)region, 0);
    for (int32_t v : slots) gone[(size_t)(v - base)] = 1;
    std::vector<int32_t> ft;   // [from | to]: only rows that change place move
    std::vector<int32_t> t2;
    int w = 0;
    for (int t = 0; t < region; ++t) {
      if (gone[(size_t)t]) continue;
      if (t != w) {
        ft.push_back(base + t);
        t2.push_back(base + w);
      }
      ++w;
    }
    if (!ft.empty()) {
      const int km = (int)ft.size();
      ft.insert(ft.end(), t2.begin(), t2.end());
      auto rows = glob_slot_rows(s, c->lp.m);
      size_t most = 0;
      for (auto &r : rows) most = r.second > most ? r.second : most;
      HIPCHK(c, s.mw_ft.ensure((size_t)km * 8));
      HIPCHK(c, s.mw_tmp.ensure((size_t)km * most));
      HIPCHK(c, hipMemcpyAsync(s.mw_ft.p, ft.data(), (size_t)km * 8, hipMemcpyHostToDevice,
                               c->stream));
      for (auto &r : rows)
        HIPCHK(c, launch_bnb_move_rows(r.first->as<unsigned char>(), s.mw_tmp.as<unsigned char>(),
                                       r.second, s.mw_ft.as<int32_t>(),
                                       s.mw_ft.as<int32_t>() + km, km, c->stream));
    }
    s.count -= k;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the staged host arrays go out of scope
  return MGPU_OK;
}

// places k device rows as open nodes in row order: on top of the stack, or
// (order 2) each in a free pool slot under the next node id
int glob_place_nodes(mgpu_ctx *c, GlobState &s, int k, const double *buf) {
  if (k == 0) return MGPU_OK;
  const int room = s.order == 2 ? s.tree.spare() : s.cap - s.count;
  if (k > room)
    return fail(c, MGPU_ERR_NOMEM, "mgpu_glob_import_dev: %d rows, the node pool has room for %d",
                k, room);
  std::vector<int32_t> slots((size_t)k);
  for (int t = 0; t < k; ++t)
    slots[(size_t)t] = s.order == 2 ? s.tree.take_slot() : s.count + t;
  GlobMigIO io;
  int rc = glob_mig_io(c, s, slots, const_cast<double *>(buf), &io);
  if (rc != MGPU_OK) return rc;
  HIPCHK(c, launch_glob_mig_unpack(io, c->stream));
  s.mw_hstage.resize((size_t)k * kMigStage);
  HIPCHK(c, hipMemcpyAsync(s.mw_hstage.data(), s.mw_stage.p, (size_t)k * kMigStage * 8,
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (s.order == 2) {
    for (int t = 0; t < k; ++t) {
      const double *h = s.mw_hstage.data() + (size_t)t * kMigStage;
      if (s.brancher >= 1) {
        GlobState::BrInfo bi;
        bi.var = (int)h[2];
        bi.isint = (int)h[3];
        bi.act = h[4];
        bi.dd = h[5];
        bi.ud = h[6];
        bi.plb = h[7];
        s.pinfo[(size_t)slots[(size_t)t]] = bi;
      }
      s.tree.push(h[0], (int)h[1], slots[(size_t)t]);
    }
  } else {
    s.count += k;
  }
  return MGPU_OK;
}

int check_glob(mgpu_ctx *c, const char *what) {
  if (!c) return MGPU_ERR_ARG;
  if (!c->glob) return fail(c, MGPU_ERR_STATE, "%s: mgpu_glob_init first", what);
  return MGPU_OK;
}

}  // namespace

// The pool-side migration workspaces for an exchange of up to S rows (a pick
// of S, an export of k <= S of them with the stack's compaction, an import
// of k <= S): sized once for that worst case (mgpu_glob_rebalance calls this
// first), so later exchanges at that S allocate nothing.
int glob_reserve_migration(mgpu_ctx *c, int S) {
  int rc = check_glob(c, "mgpu_glob_rebalance");
  if (rc != MGPU_OK) return rc;
  GlobState &s = *c->glob;
  const size_t k = (size_t)(S > 0 ? S : 1);
  size_t most = 0;
  for (auto &r : glob_slot_rows(s, c->lp.m)) most = r.second > most ? r.second : most;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, s.mw_slots.ensure(k * 4));
  HIPCHK(c, s.mw_stage.ensure(k * kMigStage * 8));
  HIPCHK(c, s.mw_ft.ensure(k * 8));
  HIPCHK(c, s.mw_tmp.ensure(k * most));
  return MGPU_OK;
}

extern "C" {

int mgpu_glob_shard(mgpu_ctx *c, int rank, int world, int *kept) {
  int rc = check_glob(c, "mgpu_glob_shard");
  if (rc != MGPU_OK) return rc;
  if (world < 1 || rank < 0 || rank >= world)
    return fail(c, MGPU_ERR_ARG, "mgpu_glob_shard: bad rank/world");
  GlobState &s = *c->glob;
  HIPCHK(c, hipSetDevice(c->device));
  glob_settle_pick(s);
  int k = 0;
  if (s.order == 2) {
    k = s.tree.shard(rank, world);
  } else {
    // stack position i from the bottom stays when i = rank (mod world): slot
    // j <- slot rank + j world, for every per-slot array
    std::vector<int32_t> ft, to;
    for (int i = rank; i < s.count; i += world, ++k)
      if (i != k) {
        ft.push_back(i);
        to.push_back(k);
      }
    if (!ft.empty()) {
      const int km = (int)ft.size();
      ft.insert(ft.end(), to.begin(), to.end());
      auto rows = glob_slot_rows(s, c->lp.m);
      size_t most = 0;
      for (auto &r : rows) most = r.second > most ? r.second : most;
      HIPCHK(c, s.mw_ft.ensure((size_t)km * 8));
      HIPCHK(c, s.mw_tmp.ensure((size_t)km * most));
      HIPCHK(c, hipMemcpyAsync(s.mw_ft.p, ft.data(), (size_t)km * 8, hipMemcpyHostToDevice,
                               c->stream));
      for (auto &r : rows)
        HIPCHK(c, launch_bnb_move_rows(r.first->as<unsigned char>(), s.mw_tmp.as<unsigned char>(),
                                       r.second, s.mw_ft.as<int32_t>(),
                                       s.mw_ft.as<int32_t>() + km, km, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
  }
  s.count = k;
  s.tot.open = k;
  if (kept) *kept = k;
  return MGPU_OK;
}

int mgpu_glob_pick(mgpu_ctx *c, int S, double *lbs, int *got) {
  int rc = check_glob(c, "mgpu_glob_pick");
  if (rc != MGPU_OK) return rc;
  if (S < 0 || (S > 0 && !lbs) || !got)
    return fail(c, MGPU_ERR_ARG, "mgpu_glob_pick: bad argument");
  GlobState &s = *c->glob;
  HIPCHK(c, hipSetDevice(c->device));
  glob_settle_pick(s);
  *got = 0;
  if (s.order == 2) {
    // TreeManager::getCandidate S times: the heap top, pruned lazily under
    // the incumbent (the pruned nodes are gone, as in a round)
    s.held = s.tree.hold(S, s.inc).nodes;
    for (size_t t = 0; t < s.held.size(); ++t) lbs[t] = s.held[t].lb;
    *got = (int)s.held.size();
    s.count = glob_open(s);
    s.tot.open = s.count;
    return MGPU_OK;
  }
  const int k = S < s.count ? S : s.count;   // the stack's top, topmost first
  if (k > 0) {
    std::vector<double> v((size_t)k);
    HIPCHK(c, hipMemcpyAsync(v.data(), s.pnlb.as<double>() + (s.count - k), (size_t)k * 8,
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int t = 0; t < k; ++t) {
      lbs[t] = v[(size_t)(k - 1 - t)];
      s.pick.push_back(s.count - 1 - t);
    }
  }
  *got = k;
  return MGPU_OK;
}

int mgpu_glob_export_dev(mgpu_ctx *c, int k, const int32_t *idx, double *buf) {
  int rc = check_glob(c, "mgpu_glob_export_dev");
  if (rc != MGPU_OK) return rc;
  GlobState &s = *c->glob;
  if (k < 0 || (k > 0 && (!idx || !buf)))
    return fail(c, MGPU_ERR_ARG, "mgpu_glob_export_dev: bad argument");
  const int np = s.order == 2 ? (int)s.held.size() : (int)s.pick.size();
  std::vector<uint8_t> seen((size_t)(np > 0 ? np : 1), 0);
  std::vector<int32_t> slots;
  for (int t = 0; t < k; ++t) {
    if (idx[t] < 0 || idx[t] >= np || seen[(size_t)idx[t]])
      return fail(c, MGPU_ERR_ARG, "mgpu_glob_export_dev: index %d is not a distinct entry of "
                  "the last mgpu_glob_pick (%d nodes)", idx[t], np);
    seen[(size_t)idx[t]] = 1;
    slots.push_back(s.order == 2 ? s.held[(size_t)idx[t]].slot : s.pick[(size_t)idx[t]]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  rc = glob_take_nodes(c, s, slots, np, buf);
  if (rc == MGPU_OK && s.order == 2) {   // the exported nodes' slots are free
    std::vector<NodeHeap::Node> stay;
    for (int t = 0; t < np; ++t) {
      if (seen[(size_t)t]) s.tree.drop(s.held[(size_t)t]);
      else stay.push_back(s.held[(size_t)t]);
    }
    s.held.swap(stay);
  }
  glob_settle_pick(s);
  s.count = glob_open(s);
  s.tot.open = s.count;
  return rc;
}

int mgpu_glob_import_dev(mgpu_ctx *c, int k, const double *buf) {
  int rc = check_glob(c, "mgpu_glob_import_dev");
  if (rc != MGPU_OK) return rc;
  if (k < 0 || (k > 0 && !buf)) return fail(c, MGPU_ERR_ARG, "mgpu_glob_import_dev: bad argument");
  GlobState &s = *c->glob;
  HIPCHK(c, hipSetDevice(c->device));
  glob_settle_pick(s);
  rc = glob_place_nodes(c, s, k, buf);
  s.count = glob_open(s);
  s.tot.open = s.count;
  return rc;
}

int mgpu_glob_row_width(mgpu_ctx *c) {
  int rc = check_glob(c, "mgpu_glob_row_width");
  if (rc != MGPU_OK) return rc;
  return (int)glob_width(c, *c->glob);
}

int mgpu_glob_count(mgpu_ctx *c, int *open, int *spare) {
  int rc = check_glob(c, "mgpu_glob_count");
  if (rc != MGPU_OK) return rc;
  const GlobState &s = *c->glob;
  if (open) *open = glob_open(s);
  if (spare) *spare = s.order == 2 ? s.tree.spare() : s.cap - s.count;
  return MGPU_OK;
}

}  // extern "C"
