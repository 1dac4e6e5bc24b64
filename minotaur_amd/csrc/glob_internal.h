// Device-side structures of the batched spatial B&B (glob_tree.hip).
#pragma once

#include "mgpu_internal.h"

namespace mgpu {

struct GlobOut {                // per round, device -> host
  long long ndec[6];            // mgpu_glob_stats decision codes
  long long lps, pivots;        // LPs solved (not pruned by K2) and their pivots
  long long br_int;             // branchings at floor / ceil (IntVarHandler)
  int nchild;                   // children written
  int best_idx;                 // batch index of the best feasible node, -1 none
  double best;
};

struct GlobIO {
  int nb, base, nv, R;
  // problem: variable types, registries, original functions (function ncon
  // is the objective when it has one; nfun = ncon + has_obj)
  const uint8_t *vtype;         // [nv]
  int nsq, nbil, ncon, nfun;
  const int32_t *sq;            // [nsq][2] x, y
  const int32_t *bil;           // [nbil][3] x0, x1, y
  const int32_t *lptr, *lvar, *qptr, *qv1, *qv2;
  const double *lval, *qval, *clb, *cub;
  double obj_const;
  double inc, abs_tol, rel_tol;
  // the round: K2 verdicts, tightened boxes and rows, LP results
  const int32_t *kinf;          // [nb] K2 infeasible (1) / failure (2, 3)
  const double *wlb, *wub;      // [nb][nv]
  const double *wrows;          // [nb][R]
  int32_t *status, *iters;      // (the separation loop merges re-solves in)
  double *obj, *x;              // [nb], [nb][nv]
  double *cand;                 // [nb][4][nv] scratch
  int32_t *dec, *bvar, *pos, *depth_in;
  double *bval;
  int8_t *bup, *bint;
  GlobOut *out;
  // the pool (stack): children go to base + pos
  double *plb, *pub, *prows, *pnlb;
  int32_t *pdepth;
  // tangent cuts of the squares (QuadHandler::separate): S slots per square,
  // T = 2 nsq S record values [2 xl, xl^2] (inactive [0, +inf]) after the R
  // row-state values of the node record wvals [nb][R + T]; pool copy ptan
  // [cap][T].  The separation loop re-solves the flagged nodes into st2 /
  // obj2 / it2 / x2 and merges them back.
  int S, T;
  double *wvals, *ptan;
  int32_t *flag, *skip2;
  const int32_t *st2, *it2;
  const double *obj2, *x2;
  unsigned long long *acc;      // [2] tangent cuts, re-solved nodes (this pass)
  const int32_t *only;          // glob_decide: only the nodes with only[b] != 0
  // the round's input nodes: depth [nb] and tangent slots [nb][T] (stack
  // order: the pool at base; reference order: gathered from pool slots)
  const int32_t *in_depth;
  const double *in_tan;
  // reference order (mgpu_glob_config order 2): the pool slots of the round
  // (gather) and of the children (2 per branched node at pos: down, up)
  const int32_t *sel, *child_slots;
  double *glb, *gub, *grows, *gtan;   // gathered boxes, rows, tangent slots
  int32_t *gdepth;
  // parent-basis warm starts (warm 1): per pool slot the parent's optimal
  // basis (head [m], statuses [n+m], has-basis flag); gathered per node;
  // the round's optimal bases (wo) go to the children
  int m, N;
  int32_t *pws_head, *ghead;
  int8_t *pws_st, *gst;
  uint8_t *pws_ok, *gok;
  const int32_t *wo_head;
  const int8_t *wo_st;
  int32_t *skip_a;              // kinf or no basis: the warm call skips the node
  // LinearHandler::presolveNode on the node's relaxation (mgpu_glob_config
  // lin 1; glob_linear): the M rows of the relaxation as a term table, rows
  // ascending, each row's terms ascending by variable.  A term's weight is
  // ltval (ltsrc < 0) or the node record's value ltsrc (< R: the rows frows,
  // else the tangent slots ftan); a row's upper side likewise (lrhsrc).
  // Column incidence lcptr / lcterm (term indices).  Objective loidx /
  // loval; has_inc: the incumbent bound inc_ub = incumbent - constant.
  int M, nobj, cons_bad, has_inc;
  double inc_ub;
  const int32_t *lrptr, *ltvar, *ltsrc, *ltrow, *lrhsrc, *lcptr, *lcterm, *loidx;
  const double *ltval, *lrlo, *lrhi, *loval;
  const double *flb_in, *fub_in, *frows, *ftan;   // the round's nodes as they come
  double *flb, *fub;            // [nb][nv] the presolved boxes (K2's input)
  int32_t *finf;                // [nb] checkBounds_ found the node infeasible
  uint8_t *fflag;               // [nb][M] the rows' BFlag
};

// ---- relstronger in lockstep (mgpu_glob_brancher 1, 2; glob_rel.hip) -------
// reliabilitySetup(20, 50, 5) (Glob.cpp:171-181): maxCands_, the strong-
// branching LP's pivot limit, the reliability threshold; StrongBrancher's eps_
constexpr int kSbCands = 20, kSbIter = 50, kSbThresh = 5;
constexpr double kSbEps = 1e-6;

// A node of the round, by its position in the round: where it stands in
// PCBProcessor::process's loop and StrongBrancher::findBranches' state.
enum RsPhase : int32_t {
  kRsDone = 0,      // decided: dec holds the node's decision
  kRsDecided = 1,   // glob_decide just ran on it: separation, then findBranches
  kRsChild = 2,     // a strong-branching child (cand cur, side) is under way
  kRsMod = 3,       // the brancher's modification: presolve, re-solve, decide
  kRsSep = 4,       // tangent cuts were added: re-solve, decide
};

struct RsNode {
  int32_t phase, pass;          // pass: the solves of the process loop so far
  int32_t cur, cnt, side;       // the candidate under way (its variable), strong-branched so far
  int32_t iend;                 // where the candidate loop stopped (variable index)
  int32_t status, mdown;        // 0 none / 1 prune / 2 mod (and its direction)
  int32_t sres[2];              // the candidate's (status, value): down, up
  int32_t dec;                  // the node's decision when done
  int32_t bc, bdir, nrel;       // best candidate, its direction (setDir; -1 unset), reliable count
  int32_t has_basis, ch_ok;     // the engine holds a basis / the children got one
  int32_t lps, sb_lps, resolves, pivots;
  int32_t o_var, o_isint, o_dir;   // the branching: variable, handler, direction
  int32_t b_var, b_isint;       // the branching that made the node (BrInfo)
  double ores[2];
  double best, minscore, last_val, objval, maxchange;
  double o_v, o_dd, o_ud;       // x_var and the candidate's distances
  double b_act, b_dd, b_ud, b_plb;
};

struct RsLog {                  // a step's main-engine solve of one node
  int32_t flag, status, iters, pad;
  double value;
};

struct RsObs {                  // one updatePCost_ call: node, variable * 2 + down
  int32_t node, vd;
  double cost;
};

// the step's read-back: counts of the nodes by what they wait for, the
// separation pass's cuts and flagged nodes, an error (1 K2 failed on a
// strong-branching child or a modification, 2 the observation log is full)
struct RsHdr {
  int32_t n_child, n_mod, n_sep, n_cold, err, err_node, nobs, pad;
  unsigned long long cuts, flagged;
};

struct RsIO {
  int obs_cap;
  double inc;                   // the round-start incumbent
  RsNode *node;                 // [nb]
  double *nlb, *nub, *nrec;     // [nb][nv], [nb][R + T]: the node's box and record
  int8_t *ck, *ci;              // [nb][nv] candidate: 0 none / 1 reliable / 2 unreliable; handler
  double *cdd, *cud, *cvio;     // [nb][nv]
  double *lpu, *lpd;            // [nb][nv] the node-local pseudocosts
  int32_t *ltu, *ltd;           // [nb][nv] and their counts
  const double *spu, *spd;      // [nv] the round-start pseudocosts
  const int32_t *stu, *std_;
  int32_t *cb_head, *ch_head;   // [nb][m] the engine's basis, the children's
  int8_t *cb_st, *ch_st;        // [nb][N]
  int32_t *skip;                // [4][nb] LP masks: child warm / cold, re-solve warm / cold
  int32_t *lst, *lit;           // [4][nb] those calls' results
  double *lobj;
  int32_t *only, *sdec;         // [nb] glob_decide's mask; glob_separate's decisions
  RsHdr *hdr;
  RsLog *log;                   // [nb] (directly after hdr)
  RsObs *obs;                   // [obs_cap]
  const int32_t *cs;            // [nb][2] children's pool slots: down, up (-1 none)
};

hipError_t launch_rs_init(const GlobIO &io, const RsIO &rs, hipStream_t stream);
hipError_t launch_rs_obbt(const GlobIO &io, const RsIO &rs, int resolve, hipStream_t stream);
hipError_t launch_rs_sdec(const GlobIO &io, const RsIO &rs, hipStream_t stream);
hipError_t launch_rs_post(const GlobIO &io, const RsIO &rs, hipStream_t stream);
hipError_t launch_rs_counts(const GlobIO &io, const RsIO &rs, hipStream_t stream);
hipError_t launch_rs_child(const GlobIO &io, const RsIO &rs, hipStream_t stream);
hipError_t launch_rs_masks(const GlobIO &io, const RsIO &rs, hipStream_t stream);
hipError_t launch_rs_absorb(const GlobIO &io, const RsIO &rs, hipStream_t stream);
hipError_t launch_rs_children(const GlobIO &io, const RsIO &rs, hipStream_t stream);

// ---- node migration between ranks (glob_migrate.hip) ------------------------
// One f64 row per node, every field exact (integers as doubles, basis
// statuses 2 bits each, 16 per double):
//   [ lb (nv) | ub (nv) | rows (R) | tan (T) | node bound | depth ]
//   warm 1:        + [ has_basis | head (m) | statuses, ceil((nv + m) / 16) ]
//   brancher >= 1: + [ var | isint | act | dd | ud | plb ]   (var -1: none)
constexpr int kMigStage = 8;    // host staging per row: bound, depth, the branching record

struct GlobMigIO {
  int k, nv, R, T, m, N, W;
  int warm, br;                 // the row carries a basis / a branching record
  const int32_t *slots;         // [k] pool slot of row t
  double *rows;                 // [k][W]
  double *plb, *pub, *prows, *ptan, *pnlb;
  int32_t *pdepth;
  int32_t *pws_head;
  int8_t *pws_st;
  uint8_t *pws_ok;
  // [k][kMigStage] = [bound | depth | var | isint | act | dd | ud | plb]: the
  // branching records live on the host per pool slot, so glob_pack reads
  // entries 2..7 from here (one upload per exchange) and glob_unpack writes
  // all eight (one download: the host's heap needs bound and depth too)
  double *stage;
};

inline size_t glob_mig_width(int nv, int R, int T, int m, int warm, int br) {
  return 2 * (size_t)nv + (size_t)R + (size_t)T + 2 +
         (warm ? 1 + (size_t)m + ((size_t)nv + (size_t)m + 15) / 16 : 0) + (br ? 6 : 0);
}

hipError_t launch_glob_mig_pack(const GlobMigIO &io, hipStream_t stream);
hipError_t launch_glob_mig_unpack(const GlobMigIO &io, hipStream_t stream);

hipError_t launch_glob_round_tail(const GlobIO &io, hipStream_t stream);
hipError_t launch_glob_decide(const GlobIO &io, hipStream_t stream);
hipError_t launch_glob_pack(const GlobIO &io, hipStream_t stream);
hipError_t launch_glob_separate(const GlobIO &io, hipStream_t stream);
hipError_t launch_glob_merge(const GlobIO &io, hipStream_t stream);
hipError_t launch_glob_gather(const GlobIO &io, hipStream_t stream);
hipError_t launch_glob_skips(const GlobIO &io, hipStream_t stream);
hipError_t launch_glob_summary(const GlobIO &io, hipStream_t stream);
hipError_t launch_glob_children(const GlobIO &io, hipStream_t stream);
hipError_t launch_glob_linear(const GlobIO &io, hipStream_t stream);
hipError_t launch_glob_linear_verdict(const GlobIO &io, hipStream_t stream);

}  // namespace mgpu
