// What the dual-simplex kernels share (K3 lp_dual.hip, K3L lp_large.hip,
// K3P lp_pfi.hip, K3PW lp_pfi_wide.hip, K3R lp_rows.hip): every one of them
// follows oracle/lp_dual.c pivot for pivot, so the tolerances, the status
// codes, the bound accessors and the oracle's small routines exist once.
#pragma once

#include "mgpu_internal.h"
#include "wave.h"

namespace mgpu {

constexpr double kPTol = 1e-7;    // primal feasibility (Clp default)
constexpr double kDTol = 1e-7;    // dual feasibility (Clp default)
constexpr double kPivTol = 1e-9;  // smallest |alpha_rq| allowed to pivot
constexpr double kArt0 = 1e7;     // first artificial box half-width
constexpr double kInfB = 1e30;    // |bound| >= this is infinite in the LP

constexpr int kUnknownStatus = 12;  // EngineUnknownStatus: node not solved

// Column status.  The dense kernels store the codes as int8_t; the
// product-form kernels pack them into an int with flag bits above (the
// enumerators promote to int there).
enum : int8_t { ST_LB = 0, ST_UB = 1, ST_FREE = 2, ST_BASIC = 3 };

// artificial bounds of a column whose finite side is thi / tlo (oracle
// place_nonbasic, grow_art)
__device__ __forceinline__ double art_lo(double thi, double ab) {
  return (thi < kInfB ? thi : 0.0) - ab;
}
__device__ __forceinline__ double art_hi(double tlo, double ab) {
  return (tlo > -kInfB ? tlo : 0.0) + ab;
}

// A nonbasic column (status st) that sits on an artificial bound (art: bit 0
// the lower, bit 1 the upper) when no row is infeasible (oracle box_state):
// kBoxGrow while its reduced cost is nonzero -- the box holds it and has to
// grow; kBoxRelease at dj = 0 -- it needs no box and goes back to its true
// bounds.  0: neither.
constexpr int kBoxGrow = 1, kBoxRelease = 2;
__device__ __forceinline__ int box_state(int st, int art, double dj) {
  if (!((st == ST_LB && (art & 1)) || (st == ST_UB && (art & 2)))) return 0;
  return fabs(dj) > kDTol ? kBoxGrow : kBoxRelease;
}

// The problem one solve sees: the node's box, the row bounds, the objective
// (ocol >= 0: osign * x[ocol], a bound LP; else c).
struct LpView {
  int n, m, N;
  const double *nlb, *nub, *rlo, *rhi, *c;
  int ocol;
  double osign;
  __device__ __forceinline__ double cj(int j) const {
    return ocol < 0 ? c[j] : (j == ocol ? osign : 0.0);
  }
  __device__ __forceinline__ double tlo(int j) const {
    const double v = j < n ? nlb[j] : rlo[j - n];
    return v < -kInfB ? -INFINITY : v;
  }
  __device__ __forceinline__ double thi(int j) const {
    const double v = j < n ? nub[j] : rhi[j - n];
    return v > kInfB ? INFINITY : v;
  }
};

// The constraint matrix in CSC (pivot row rho'A, FTRAN) and CSR (primal
// recompute).
struct LpMat {
  const int *colptr, *rowidx, *rowptr, *ccol;
  const double *cval, *rval;
};

// rho' a_j over CSC column j in CSC order; four entries' loads are issued
// before their products are summed (the adds keep the sequential order)
__device__ __forceinline__ double col_dot(const LpMat &A, const double *rho, int j) {
  double a = 0.0;
  int t = A.colptr[j];
  const int e = A.colptr[j + 1];
  for (; t + 4 <= e; t += 4) {
    const int i0 = A.rowidx[t], i1 = A.rowidx[t + 1], i2 = A.rowidx[t + 2], i3 = A.rowidx[t + 3];
    const double v0 = A.cval[t], v1 = A.cval[t + 1], v2 = A.cval[t + 2], v3 = A.cval[t + 3];
    const double r0 = rho[i0], r1 = rho[i1], r2 = rho[i2], r3 = rho[i3];
    a += v0 * r0;
    a += v1 * r1;
    a += v2 * r2;
    a += v3 * r3;
  }
  for (; t < e; ++t) a += A.cval[t] * rho[A.rowidx[t]];
  return a;
}

// ---- the matrix in LDS (K3, K3P, K3PW) --------------------------------------
// colptr, rowidx, cval, rowptr, ccol, rval in this order, each 16-B aligned
__host__ __device__ inline size_t lp_matrix_bytes(int n, int m, int nnz) {
  return al16((size_t)(n + 1) * 4) + al16((size_t)nnz * 4) + al16((size_t)nnz * 8) +
         al16((size_t)(m + 1) * 4) + al16((size_t)nnz * 4) + al16((size_t)nnz * 8);
}

// Carves the six arrays at p (advancing it past them) and stages them with
// the workgroup's T threads; the caller's barrier publishes them.
template <int T>
__device__ __forceinline__ LpMat stage_matrix(unsigned char *&p, const DevLP &lp) {
  const int n = lp.n, m = lp.m, nnz = lp.nnz;
  int *s_colptr = (int *)p;      p += al16((size_t)(n + 1) * 4);
  int *s_rowidx = (int *)p;      p += al16((size_t)nnz * 4);
  double *s_cval = (double *)p;  p += al16((size_t)nnz * 8);
  int *s_rowptr = (int *)p;      p += al16((size_t)(m + 1) * 4);
  int *s_ccol = (int *)p;        p += al16((size_t)nnz * 4);
  double *s_rval = (double *)p;  p += al16((size_t)nnz * 8);
  for (int t = threadIdx.x; t <= n; t += T) s_colptr[t] = lp.colptr[t];
  for (int t = threadIdx.x; t <= m; t += T) s_rowptr[t] = lp.rowptr[t];
  for (int t = threadIdx.x; t < nnz; t += T) {
    s_rowidx[t] = lp.rowidx[t];
    s_cval[t] = lp.cval[t];
    s_ccol[t] = lp.ccol[t];
    s_rval[t] = lp.rval[t];
  }
  return LpMat{s_colptr, s_rowidx, s_rowptr, s_ccol, s_cval, s_rval};
}

// ---- node list, per-node rows, unsolved nodes (K3, K3L) ---------------------
// (node_rows_overlay, working_bounds and place_columns are called by K3L;
// K3 keeps the same loops written out, marked there: as calls its LP step
// with per-node rows measured 0.46 % slower.)
// The list positions a launch solves: [lo, nsolve) of node_list (the
// product-form kernels' overflow re-solve: list_lo .. min(*node_count,
// list_hi)), or the whole batch.
__device__ __forceinline__ void node_range(const LpIO &io, int &lo, int &nsolve) {
  lo = io.node_list != nullptr ? io.list_lo : 0;
  nsolve = io.batch;
  if (io.node_list != nullptr) {
    nsolve = *io.node_count;
    if (nsolve > io.list_hi) nsolve = io.list_hi;
  }
}

// Node b's matrix values and row bounds into wc / wr / wlo / whi: the loaded
// values (A0, rlo0, rhi0), then the node's own entries (OsiLPEngine::
// changeConstraint of the rewritten rows); A and V then read the copy.  Run
// by threads t0, t0 + stride, ... of the group that owns the copy; sync()
// orders that group's writes.
template <class Sync>
__device__ __forceinline__ void node_rows_overlay(LpMat &A, LpView &V, const LpMat &A0,
                                                  const double *rlo0, const double *rhi0,
                                                  const NodeRowsIO &nr, int b, int nnz, double *wc,
                                                  double *wr, double *wlo, double *whi, int t0,
                                                  int stride, Sync sync) {
  for (int t = t0; t < nnz; t += stride) {
    wc[t] = A0.cval[t];
    wr[t] = A0.rval[t];
  }
  for (int i = t0; i < V.m; i += stride) {
    wlo[i] = rlo0[i];
    whi[i] = rhi0[i];
  }
  sync();
  const double *rec = nr.vals + (size_t)b * nr.stride;
  for (int q = t0; q < nr.ncoef; q += stride) {
    double v = rec[nr.coef_src[q]];
    if (fabs(v) <= kLfTol) v = 0.0;
    wc[nr.csc_pos[q]] = v;
    wr[nr.csr_pos[q]] = v;
  }
  for (int q = t0; q < nr.nrow; q += stride) {
    const int r = nr.row[q];
    if (nr.lo_src[q] >= 0) wlo[r] = rec[nr.lo_src[q]];
    if (nr.hi_src[q] >= 0) whi[r] = rec[nr.hi_src[q]];
  }
  sync();
  A.cval = wc;
  A.rval = wr;
  V.rlo = wlo;
  V.rhi = whi;
}

// A node that is not solved (skipped: kUnknownStatus; empty box: 2); one
// thread of the node's group calls it.
__device__ __forceinline__ void write_unsolved(const LpIO &io, int b, int status) {
  io.status[b] = status;
  io.obj[b] = INFINITY;
  io.iters[b] = 0;
}

// ---- dense-kernel column state (K3's Ctx, K3L's S<kT>) ----------------------
// CS has the LpView plus d, z, blo, bhi (double) and st, art (int8_t) per
// column; loops run over columns t0, t0 + stride, ...

// working bounds; true for a thread that saw an empty box (infeasible before
// any pivot)
template <class CS>
__device__ __forceinline__ bool working_bounds(const CS &s, int t0, int stride) {
  bool bad = false;
  for (int j = t0; j < s.N; j += stride) {
    s.blo[j] = s.tlo(j);
    s.bhi[j] = s.thi(j);
    s.art[j] = 0;
    bad |= s.blo[j] > s.bhi[j] + kPTol;
  }
  return bad;
}

// oracle place_nonbasic
template <class CS>
__device__ __forceinline__ void place_nonbasic(const CS &s, int j, double ab) {
  const double lo = s.blo[j], hi = s.bhi[j], dj = s.d[j];
  const bool lo_f = lo > -kInfB, hi_f = hi < kInfB;
  if (lo_f && hi_f && lo == hi) {
    s.st[j] = ST_LB;
    s.z[j] = lo;
    return;
  }
  if (dj > kDTol) {
    if (!lo_f) {
      s.blo[j] = art_lo(hi, ab);
      s.art[j] |= 1;
    }
    s.st[j] = ST_LB;
    s.z[j] = s.blo[j];
  } else if (dj < -kDTol) {
    if (!hi_f) {
      s.bhi[j] = art_hi(lo, ab);
      s.art[j] |= 2;
    }
    s.st[j] = ST_UB;
    s.z[j] = s.bhi[j];
  } else if (lo_f) {
    s.st[j] = ST_LB;
    s.z[j] = lo;
  } else if (hi_f) {
    s.st[j] = ST_UB;
    s.z[j] = hi;
  } else {
    s.st[j] = ST_FREE;
    s.z[j] = 0.0;
  }
}

// nonbasic placement: a warm start keeps a column's status when it is dual
// feasible there; every other column goes through place_nonbasic
template <class CS>
__device__ __forceinline__ void place_columns(const CS &s, bool warm, double ab, int t0,
                                              int stride) {
  for (int j = t0; j < s.N; j += stride) {
    if (s.st[j] == ST_BASIC) continue;
    const double lo = s.blo[j], hi = s.bhi[j], dj = s.d[j];
    bool keep = false;
    if (warm) {
      const int8_t v = s.st[j];
      if (v == ST_LB && lo > -kInfB && dj >= -kDTol) {
        s.z[j] = lo;
        keep = true;
      } else if (v == ST_UB && hi < kInfB && dj <= kDTol) {
        s.z[j] = hi;
        keep = true;
      } else if (lo == hi && lo > -kInfB) {
        s.st[j] = ST_LB;
        s.z[j] = lo;
        keep = true;
      }
    }
    if (!keep) place_nonbasic(s, j, ab);
  }
}

// oracle release_art
template <class CS>
__device__ __forceinline__ void release_art(const CS &s, int t0, int stride) {
  for (int j = t0; j < s.N; j += stride) {
    if (box_state(s.st[j], s.art[j], s.d[j]) != kBoxRelease) continue;
    s.blo[j] = s.tlo(j);
    s.bhi[j] = s.thi(j);
    s.art[j] = 0;
    place_nonbasic(s, j, 0.0);
  }
}

// oracle grow_art
template <class CS>
__device__ __forceinline__ void grow_art(const CS &s, double ab, int t0, int stride) {
  for (int j = t0; j < s.N; j += stride) {
    const int8_t a = s.art[j];
    if (!a || s.st[j] == ST_BASIC) continue;
    if (a & 1) s.blo[j] = art_lo(s.thi(j), ab);
    if (a & 2) s.bhi[j] = art_hi(s.tlo(j), ab);
    if (s.st[j] == ST_LB) s.z[j] = s.blo[j];
    if (s.st[j] == ST_UB) s.z[j] = s.bhi[j];
  }
}

}  // namespace mgpu
