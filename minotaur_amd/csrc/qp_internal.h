// Device-side structures of the batched QP relaxation solve (qp_kkt.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mgpu {

constexpr double kQpTolMu = 1e-10;   // complementarity (oracle/qp_ipm.py TOL_MU)
constexpr double kQpTolP = 1e-9;     // primal residual, relative (oracle/qp_ipm.py TOL_P)
constexpr double kQpReg = 1e-12;     // relative regularisation of M
constexpr double kQpStep = 0.995;    // fraction to the boundary

struct DevQP {
  int n, m, np, mp;          // sizes and their multiples of 16
  const double *Q;           // [np][np] symmetric, zero padded
  const double *c;           // [np]
  const double *A;           // [mp][np]
  const double *AT;          // [np][mp]
  const double *b;           // [mp]
  double k;                  // objective constant
  double tp, td;             // primal / dual residual tolerances
};

struct QpWork {
  int B;
  int rule;                  // launch-uniform step rule of qp_step: 0 separate primal and
                             // dual step lengths, 1 one common length min(ap, ad)
  const int32_t *skip;       // [B] or null: nonzero = not solved (status 12, obj +inf)
  double *l, *u;             // [B][np] node boxes (padding fixed at 0)
  double *x, *zl, *zu;       // [B][np]
  double *y;                 // [B][mp]
  double *rd;                // [B][np]
  double *rp;                // [B][mp]
  double *K;                 // [B][np][np]
  double *W;                 // [B][np][mp]
  double *WT;                // [B][mp][np] (W', for W dy)
  double *M;                 // [B][mp][mp]
  int32_t *done, *iters, *status;
  double *obj;
};

// Which kernels one interior-point iteration takes at a padded shape: the
// one place the LDS budgets of qp_kkt.hip's variants are weighed.
struct QpPlan {
  bool ll;   // qp_potrf_ll (left-looking Cholesky); else qp_potrf
  bool wl;   // qp_trsm_syrk_lds (W resident in LDS); else qp_trsm_syrk
  int J;     // columns per thread of qp_step<J>: 2, 4 or 8
  bool ok;   // every chosen kernel can be launched; mgpu_load_qp refuses the rest
};
QpPlan qp_plan(int np, int mp, int m);

size_t qp_step_lds(int np, int mp, int m);
hipError_t launch_qp_init(const DevQP &q, const QpWork &w, hipStream_t s);
// ev (optional): four events recorded before the factor kernel, after it,
// after the W / Schur kernel and after the step kernel
hipError_t launch_qp_iteration(const DevQP &q, const QpWork &w, hipStream_t s,
                               hipEvent_t *ev = nullptr);
hipError_t launch_qp_iteration_check(const DevQP &q, const QpWork &w, hipStream_t s);
hipError_t launch_qp_final(const DevQP &q, const QpWork &w, hipStream_t s);

// The retry's compact batch (mgpu_qp_step_rule 2).  Gather: the nodes b of the
// round with mask[b] != 0, in their order, into idx[0 .. k), their boxes
// ([B][n], unpadded) into cl / cu [k][n], and k into *count.  Scatter: the
// compact batch's results in w (status, obj, iters + it_add, x [k][np]) to the
// slots idx names of status / obj / iters / x ([B][n], may be null).
hipError_t launch_qp_retry_gather(const int32_t *mask, int B, int n, const double *lb,
                                  const double *ub, int32_t *idx, int32_t *count, double *cl,
                                  double *cu, hipStream_t s);
hipError_t launch_qp_retry_scatter(const QpWork &w, int k, int n, int np, const int32_t *idx,
                                   int it_add, int32_t *status, double *obj, int32_t *iters,
                                   double *x, hipStream_t s);

}  // namespace mgpu
