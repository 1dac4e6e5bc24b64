// The column side of the product-form dual simplex, shared by K3P
// (lp_pfi.hip, one basis row per lane) and K3PW (lp_pfi_wide.hip, two):
// everything indexed by column j = s*64 + lane (slot s < S of that lane,
// N = n + m <= 64*S) is the same code in both.  Reduced cost d, pivot-row
// entry al, Harris pass-2 ratio t2, working-bound copies tl / th and the
// packed status sa are per-slot registers; the column values zc and working
// bounds lo / hi are the wave's LDS slice.  The arithmetic is oracle/
// lp_dual.c's, loop for loop.  The row side (BTRAN, FTRAN, primals, the eta
// file, reinversion) stays in each kernel.
//
// Two of the functions, pfi_working_bounds and pfi_harris2, are called by
// K3PW only: K3P keeps the same loops written out (marked there), because
// with both as calls its S = 3, 32-eta build -- 128 VGPRs with a deliberate
// spill -- grew from 92 to 100 B of scratch per lane.  A change to either
// loop is made in both places.
#pragma once

#include "lp_common.h"

namespace mgpu {

// packed column status: bits 0-1 status, 2-3 artificial-bound flags, 4 fixed
constexpr int kArtLo = 4, kArtHi = 8, kFixed = 16;

struct PfiProb : LpMat, LpView {
  const double *b0;  // (B0^{-1})_{ik} = b0[k*ld + i]
  int ld;
};

// the warm start every node of the launch shares, staged once per workgroup
struct PfiWarm {
  double *b0;   // B0^{-1}, column-major with the odd leading dimension m + 1
  double *wd;   // reduced costs [N]
  int *wst;     // statuses [N]: basic = in head
  int *whead;   // basic column per row [m]
};
__host__ __device__ inline size_t pfi_warm_bytes(int n, int m) {
  const int N = n + m;
  return al16((size_t)m * (m + 1) * 8) + al16((size_t)N * 8) + al16((size_t)N * 4) +
         al16((size_t)m * 4);
}

// Carves the warm start at p (advancing it past the four arrays) and stages
// it with the workgroup's T threads; pfi_mark_basic completes it.
template <int T>
__device__ __forceinline__ PfiWarm pfi_stage_warm(unsigned char *&p, const LpWarm &ws, int n,
                                                  int m) {
  const int N = n + m, ld = m + 1;
  PfiWarm w;
  w.b0 = (double *)p;  p += al16((size_t)m * ld * 8);
  w.wd = (double *)p;  p += al16((size_t)N * 8);
  w.wst = (int *)p;    p += al16((size_t)N * 4);
  w.whead = (int *)p;  p += al16((size_t)m * 4);
  for (int t = threadIdx.x; t < m * m; t += T)  // ABI: column-major, t = k*m + i
    w.b0[(t / m) * ld + t % m] = ws.binv[t];
  for (int t = threadIdx.x; t < N; t += T) {
    w.wd[t] = ws.d != nullptr ? ws.d[t] : 0.0;  // bound LPs rebuild d
    const int8_t s = ws.st[t];
    w.wst[t] = s == ST_BASIC ? ST_LB : s;
  }
  for (int t = threadIdx.x; t < m; t += T) w.whead[t] = ws.head[t];
  return w;
}
// publishes everything staged so far and marks the head's columns basic
template <int T>
__device__ __forceinline__ void pfi_mark_basic(const PfiWarm &w, int m) {
  __syncthreads();
  for (int t = threadIdx.x; t < m; t += T) w.wst[w.whead[t]] = ST_BASIC;  // basic = in head
  __syncthreads();
}

// Working bounds into tl / th and the LDS slice, the start status
// start_st(j) into sa (slots past N act as basic: never touched).  True
// when some column's box is empty: infeasible before any pivot.
template <int S, class St>
__device__ __forceinline__ bool pfi_working_bounds(const PfiProb &P, St start_st, double *lo,
                                                   double *hi, int lane, double (&tl)[S],
                                                   double (&th)[S], int (&sa)[S]) {
  bool bad = false;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int j = s * 64 + lane;
    const bool valid = j < P.N;
    tl[s] = valid ? P.tlo(j) : 0.0;
    th[s] = valid ? P.thi(j) : 0.0;
    sa[s] = valid ? start_st(j) : ST_BASIC;
    bad |= valid && tl[s] > th[s] + kPTol;
    if (valid) {
      lo[j] = tl[s];
      hi[j] = th[s];
    }
  }
  return __any(bad);
}

// nonbasic placement: keep the warm status when dual feasible
template <int S>
__device__ __forceinline__ void pfi_place(const PfiProb &P, int (&sa)[S], const double (&d)[S],
                                          const double (&tl)[S], const double (&th)[S],
                                          double *zc, double *lo, double *hi, int lane,
                                          double art_bound) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int j = s * 64 + lane;
    if (j >= P.N) continue;
    if (sa[s] == ST_BASIC) {  // the fixed bit matters once it leaves the basis
      zc[j] = 0.0;
      sa[s] = ST_BASIC | (tl[s] == th[s] ? kFixed : 0);
      continue;
    }
    double lo_j = tl[s], hi_j = th[s], z;
    const double dj = d[s];
    const bool lo_f = lo_j > -kInfB, hi_f = hi_j < kInfB;
    int st = sa[s], art = 0;
    if (st == ST_LB && lo_f && dj >= -kDTol) {
      z = lo_j;
    } else if (st == ST_UB && hi_f && dj <= kDTol) {
      z = hi_j;
    } else if (lo_j == hi_j && lo_f) {
      st = ST_LB;
      z = lo_j;
    } else if (dj > kDTol) {  // oracle place_nonbasic
      if (!lo_f) {
        lo_j = art_lo(hi_j, art_bound);
        lo[j] = lo_j;
        art = kArtLo;
      }
      st = ST_LB;
      z = lo_j;
    } else if (dj < -kDTol) {
      if (!hi_f) {
        hi_j = art_hi(lo_j, art_bound);
        hi[j] = hi_j;
        art = kArtHi;
      }
      st = ST_UB;
      z = hi_j;
    } else if (lo_f) {
      st = ST_LB;
      z = lo_j;
    } else if (hi_f) {
      st = ST_UB;
      z = hi_j;
    } else {
      st = ST_FREE;
      z = 0.0;
    }
    zc[j] = z;
    sa[s] = st | art | (lo_j == hi_j ? kFixed : 0);
  }
}

// oracle grow_art
template <int S>
__device__ __forceinline__ void pfi_grow(const PfiProb &P, int (&sa)[S], double *zc, double *lo,
                                         double *hi, int lane, double ab) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int j = s * 64 + lane;
    const int st = sa[s] & 3;
    if (!(sa[s] & (kArtLo | kArtHi)) || st == ST_BASIC) continue;
    double lo_j = lo[j], hi_j = hi[j];
    if (sa[s] & kArtLo) lo_j = lo[j] = art_lo(P.thi(j), ab);
    if (sa[s] & kArtHi) hi_j = hi[j] = art_hi(P.tlo(j), ab);
    if (st == ST_LB) zc[j] = lo_j;
    if (st == ST_UB) zc[j] = hi_j;
    sa[s] = (sa[s] & ~kFixed) | (lo_j == hi_j ? kFixed : 0);
  }
}

// What the nonbasic columns on an artificial bound ask for before the basis
// counts as optimal (box_state over every column): kBoxGrow | kBoxRelease
static_assert(kArtLo == 1 << 2 && kArtHi == 2 << 2, "box_state reads the flags as bits 0 and 1");
template <int S>
__device__ __forceinline__ int pfi_box_state(const int (&sa)[S], const double (&d)[S]) {
  int box = 0;
#pragma unroll
  for (int s = 0; s < S; ++s) box |= box_state(sa[s] & 3, (sa[s] >> 2) & 3, d[s]);
  return (__any(box & kBoxGrow) ? kBoxGrow : 0) | (__any(box & kBoxRelease) ? kBoxRelease : 0);
}

// oracle release_art
template <int S>
__device__ __forceinline__ void pfi_release(int (&sa)[S], const double (&d)[S], double *zc,
                                            double *lo, double *hi, int lane) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int j = s * 64 + lane;
    if (box_state(sa[s] & 3, (sa[s] >> 2) & 3, d[s]) != kBoxRelease) continue;
    // the artificial side's true bound is infinite; the other side kept its
    // own, where place_nonbasic puts a zero reduced cost when it is finite
    const bool at_lo = (sa[s] & 3) == ST_LB;
    (at_lo ? lo : hi)[j] = at_lo ? -INFINITY : INFINITY;
    const double o = (at_lo ? hi : lo)[j];
    const bool o_f = fabs(o) < kInfB;
    sa[s] = o_f ? (at_lo ? ST_UB : ST_LB) : ST_FREE;
    zc[j] = o_f ? o : 0.0;
  }
}

// some nonbasic column has an artificial bound (dual unbounded: grow or stop)
template <int S>
__device__ __forceinline__ bool pfi_any_boxed(const int (&sa)[S]) {
  bool boxed = false;
#pragma unroll
  for (int s = 0; s < S; ++s)
    boxed |= (sa[s] & 3) != ST_BASIC && (sa[s] & (kArtLo | kArtHi)) != 0;
  return __any(boxed);
}

// Pivot row al = rho'A (rho: the wave's LDS slice) and Harris pass 1; the
// pass-2 ratio is kept per slot in t2 (+inf for columns that cannot enter).
// Returns the lane's smallest relaxed ratio.  The ratios without divergent
// branches: one numerator pair and denominator per case, two divisions for
// every lane (the same operands as the per-case formulas, so the same
// values).
template <int S>
__device__ __forceinline__ double pfi_harris1(const PfiProb &P, const double *rho, double sigma,
                                              const int (&sa)[S], const double (&d)[S],
                                              double (&al)[S], double (&t2)[S], int lane) {
  double tmax = INFINITY;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int j = s * 64 + lane;
    double a = 0.0, tt = INFINITY;
    const int st = sa[s] & 3;
    if (st != ST_BASIC && !(sa[s] & kFixed)) {
      a = j >= P.n ? -rho[j - P.n] : col_dot(P, rho, j);
      const double at = sigma * a, dj = d[s], fat = fabs(at);
      const bool lb = st == ST_LB && at > kPivTol, ub = st == ST_UB && at < -kPivTol,
                 fr = st == ST_FREE && fat > kPivTol;
      const double n2 = lb ? fmax(dj, 0.0) : ub ? fmin(dj, 0.0) : 0.0;
      const double n1 = lb ? n2 + kDTol : ub ? n2 - kDTol : kDTol;
      const double den = fr ? fat : at;
      if (lb || ub || fr) {
        const double tr = n1 / den;
        tt = fr ? 0.0 : n2 / den;
        if (tr < tmax) tmax = tr;
      }
    }
    al[s] = a;
    t2[s] = tt;
  }
  return tmax;
}

// Harris pass 2: the entering column q = largest |alpha| among ratios <=
// tmax (lowest column on ties), qa its |alpha| (0: none); the owner lane
// keeps its candidate's reduced cost, alpha and status bits in cd / cal / csa
template <int S>
__device__ __forceinline__ void pfi_harris2(const int (&sa)[S], const double (&d)[S],
                                            const double (&al)[S], const double (&t2)[S],
                                            double tmax, int lane, double &qa, int &q, double &cd,
                                            double &cal, int &csa) {
  qa = 0.0, cd = 0.0, cal = 0.0;
  q = INT_MAX, csa = 0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (t2[s] <= tmax) {
      const double fa = fabs(al[s]);
      if (fa > qa) {
        qa = fa;
        q = s * 64 + lane;
        cd = d[s];
        cal = al[s];
        csa = sa[s];
      }
    }
  }
  wave_argmax_idx(qa, q);
}

// The column side of a pivot: column q (candidate data cd / cal / csa on its
// owner lane) enters with dual step theta_d, column pl leaves to the bound it
// violated (delta < 0: lower).  d -= theta_d al on the nonbasic columns, the
// two status swaps, and lane 0's writes of zc / lo / hi.  Out: the entering
// column's new value zq and its bounds as a basic column, bloq / bhiq.
template <int S>
__device__ __forceinline__ void pfi_pivot_cols(const PfiProb &P, int (&sa)[S], double (&d)[S],
                                               const double (&al)[S], double *zc, double *lo,
                                               double *hi, int lane, int q, int pl, double cd,
                                               double cal, int csa, double sigma, double delta,
                                               double theta_p, double &zq, double &bloq,
                                               double &bhiq) {
  const int ql = q & 63, qs = q >> 6;
  double theta_d = rld(cd, ql) / rld(cal, ql);
  if (sigma * theta_d < 0) theta_d = 0.0;
  const int pls = pl >> 6, pll = pl & 63;
#pragma unroll
  for (int s = 0; s < S; ++s)
    if ((sa[s] & 3) != ST_BASIC) d[s] -= theta_d * al[s];
  zq = zc[q] + theta_p;
  const bool art_q = (rl(csa, ql) & (kArtLo | kArtHi)) != 0;
  bloq = lo[q], bhiq = hi[q];
  const double bound_p = delta < 0 ? lo[pl] : hi[pl];
  wave_sync();
  if (art_q) {  // basic columns keep their true (infinite) bounds
    bloq = P.tlo(q);
    bhiq = P.thi(q);
  }
  if (lane == 0) {
    zc[q] = 0.0;        // basic now (its value is zB of row r)
    zc[pl] = bound_p;   // leaving column to its violated bound
    lo[q] = bloq;
    hi[q] = bhiq;
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (s == qs && lane == ql) {
      d[s] = 0.0;
      sa[s] = ST_BASIC | (bloq == bhiq ? kFixed : 0);
    }
    if (s == pls && lane == pll) {
      d[s] = -theta_d;
      sa[s] = (delta < 0 ? ST_LB : ST_UB) | (sa[s] & kFixed);
    }
  }
}

// statuses and reduced costs of an overflowing node into continuation slot
// `slot` (the dense kernel goes on from them)
template <int S>
__device__ __forceinline__ void pfi_write_cont(const PfiIO &px, int slot, int N,
                                               const int (&sa)[S], const double (&d)[S],
                                               int lane) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int j = s * 64 + lane;
    if (j < N) {
      px.c_st[(size_t)slot * N + j] = (int8_t)(sa[s] & 3);
      px.c_d[(size_t)slot * N + j] = d[s];
    }
  }
}

}  // namespace mgpu
