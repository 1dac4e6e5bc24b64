/*
 * CPU model for K1's changed-column skip (tools/k1_cols_model.py): the
 * project's oracle/fbbt_linear.c (simplePresolve in node mode) restated with
 *   - a clean column per node (-1: nothing known), and
 *   - per sweep the set of columns whose bounds a row visit or the objective
 *     stored in that sweep (plus the clean column in the first sweep, or every
 *     column when the node has none): the set K1 marks in its LDS words.
 * With skip != 0, tightenInts_ and checkBounds_ take only the columns of that
 * set; with skip == 0 they take every column, as the oracle does.  The sets
 * are recorded in both runs, so the caller can compare the four outputs of
 * the two runs node by node and count the column visits either way.
 * n <= 128.  Same arithmetic and order as oracle/fbbt_linear.c; compile with
 * -ffp-contract=off.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define INT_TOL 1e-6
#define E_TOL 1e-8
#define INFTY 1e20
#define MAX_SWEEPS 10

typedef struct {
  int n, m, nobj, cons_bad;
  const int *rowptr, *colidx, *colptr, *rowidx, *vtype, *objidx;
  const double *val, *rlo, *rhi, *objval;
} prob;

typedef struct {
  const prob *P;
  double *lb, *ub;
  unsigned char *flag;
  int nmods;
  unsigned nintmods;
  uint64_t set[2];   /* columns stored since the last column pass */
} node;

static int is_int(int t) { return t == 0 || t == 1; }
static void mark(node *s, int j) { s->set[j >> 6] |= 1ull << (j & 63); }
static int in_set(const node *s, int j) { return (int) ((s->set[j >> 6] >> (j & 63)) & 1ull); }

static void change_bflag(node *s, int j)
{
  for (int k = s->P->colptr[j]; k < s->P->colptr[j + 1]; ++k) s->flag[s->P->rowidx[k]] = 1;
}

static void lf_bnds(const node *s, int nt, const int *idx, const double *a, double *lo, double *up)
{
  double l = 0, u = 0;
  for (int t = 0; t < nt; ++t) {
    double c = a[t], vl = s->lb[idx[t]], vu = s->ub[idx[t]];
    if (c > 0) { l += c * vl; u += c * vu; } else { l += c * vu; u += c * vl; }
  }
  *lo = l; *up = u;
}

static void sing_lf_bnds(const node *s, int nt, const int *idx, const double *a, double *lo,
                         double *up)
{
  double l = 0, u = 0;
  int lo_sing = 0, up_sing = 0, lo_fin = 1, up_fin = 1;
  for (int t = 0; t < nt; ++t) {
    double c = a[t], vl = s->lb[idx[t]], vu = s->ub[idx[t]];
    if (c > E_TOL) {
      if (vu < INFTY && up_fin) u += c * vu;
      else if (up_sing) { up_sing = 0; u = INFINITY; up_fin = 0; }
      else up_sing = 1;
      if (vl > -INFTY && lo_fin) l += c * vl;
      else if (lo_sing) { lo_sing = 0; l = -INFINITY; lo_fin = 0; }
      else lo_sing = 1;
    } else if (c < -E_TOL) {
      if (vu < INFTY && lo_fin) l += c * vu;
      else if (lo_sing) { lo_sing = 0; l = -INFINITY; lo_fin = 0; }
      else lo_sing = 1;
      if (vl > -INFTY && up_fin) u += c * vl;
      else if (up_sing) { up_sing = 0; u = INFINITY; up_fin = 0; }
      else up_sing = 1;
    }
  }
  *lo = l; *up = u;
}

/* updateLfBoundsFromLb_ (from_lb) / updateLfBoundsFromUb_ with diff = side - activity */
static void upd(node *s, int nt, const int *idx, const double *a, double diff, int from_lb,
                int is_sing, int *changed, int count_int)
{
  for (int t = 0; t < nt; ++t) {
    int j = idx[t];
    double c = a[t], vlb = s->lb[j], vub = s->ub[j];
    if (!(c > E_TOL || c < -E_TOL)) continue;
    int low = from_lb ? c > 0 : c < 0;   /* raises the lower bound */
    if (low) {
      if (is_sing && !(vub >= INFTY)) continue;
      if (vub >= INFTY) vub = 0.;
      double nlb = diff / c + vub;
      if (nlb > vlb + E_TOL) {
        if (nlb > s->ub[j] - E_TOL) nlb = s->ub[j];
        change_bflag(s, j);
        s->lb[j] = nlb;
        mark(s, j);
        s->nmods++;
        if (count_int && is_int(s->P->vtype[j])) s->nintmods++;
        *changed = 1;
      }
    } else {
      if (is_sing && !(vlb <= -INFTY)) continue;
      if (vlb <= -INFTY) vlb = 0.;
      double nub = diff / c + vlb;
      if (nub < vub - E_TOL) {
        if (nub < s->lb[j] + E_TOL) nub = s->lb[j];
        change_bflag(s, j);
        s->ub[j] = nub;
        mark(s, j);
        s->nmods++;
        if (count_int && is_int(s->P->vtype[j])) s->nintmods++;
        *changed = 1;
      }
    }
  }
}

static int lin_bnd_tighten(node *s, int i, int *changed)
{
  const prob *P = s->P;
  int nt = P->rowptr[i + 1] - P->rowptr[i];
  const int *idx = P->colidx + P->rowptr[i];
  const double *a = P->val + P->rowptr[i];
  double lb = P->rlo[i], ub = P->rhi[i], ll, uu, sing_ll = -INFINITY, sing_uu = INFINITY;
  *changed = 0;
  lf_bnds(s, nt, idx, a, &ll, &uu);
  if (ll < -INFTY || uu > INFTY) sing_lf_bnds(s, nt, idx, a, &sing_ll, &sing_uu);
  if (ll > ub + E_TOL) return 1;
  if (uu < lb - E_TOL) return 1;
  if (lb > -INFTY) {
    if (uu < INFTY) upd(s, nt, idx, a, lb - uu, 1, 0, changed, 1);
    else if (sing_uu < INFTY) upd(s, nt, idx, a, lb - sing_uu, 1, 1, changed, 1);
  }
  if (*changed) {
    lf_bnds(s, nt, idx, a, &ll, &uu);
    if (ll < -INFTY || uu > INFTY) sing_lf_bnds(s, nt, idx, a, &sing_ll, &sing_uu);
  }
  if (ub < INFTY) {
    if (ll > -INFTY) upd(s, nt, idx, a, ub - ll, 0, 0, changed, 1);
    else if (sing_ll > -INFTY) upd(s, nt, idx, a, ub - sing_ll, 0, 1, changed, 1);
  }
  return 0;
}

static void bnds_from_obj(node *s, double ub, int *changed)
{
  const prob *P = s->P;
  int tch = 1;
  long guard = 0;
  if (P->nobj <= 0) return;
  while (tch) {
    double ll, uu, sing_ll = INFINITY, sing_uu = INFINITY;
    tch = 0;
    lf_bnds(s, P->nobj, P->objidx, P->objval, &ll, &uu);
    if (ll < -INFTY || uu > INFTY) sing_lf_bnds(s, P->nobj, P->objidx, P->objval, &sing_ll, &sing_uu);
    if (ll > ub + E_TOL) return;
    if (ll > -INFTY) upd(s, P->nobj, P->objidx, P->objval, ub - ll, 0, 0, &tch, 0);
    else if (sing_ll > -INFTY) upd(s, P->nobj, P->objidx, P->objval, ub - sing_ll, 0, 1, &tch, 0);
    if (tch) *changed = 1;
    if (++guard > 100000L) break;
  }
}

/* One node.  sets[2 * sweep], sets[2 * sweep + 1]: the set the sweep's column
 * pass sees; *nsweeps: sweeps run.  Returns infeasible. */
static int fbbt_node(const prob *P, double *lb, double *ub, int has_inc, double inc_ub,
                     unsigned char *flag, int clean_col, int skip, int *nmods_out,
                     uint64_t *sets, int *nsweeps)
{
  node s;
  int changed = 1, infeas = 0;
  unsigned iters = 1;
  s.P = P; s.lb = lb; s.ub = ub; s.flag = flag; s.nmods = 0; s.nintmods = 0;
  s.set[0] = s.set[1] = 0;
  if (clean_col >= 0 && clean_col < P->n) mark(&s, clean_col);
  else s.set[0] = s.set[1] = ~0ull;
  memset(flag, 1, (size_t) P->m);
  *nsweeps = 0;
  while (changed && iters <= 10 && (iters <= 2 || s.nintmods > 0) && !infeas) {
    s.nintmods = 0;
    changed = 0;
    ++iters;
    for (int i = 0; i < P->m; ++i) {
      if (s.flag[i]) {
        int tch;
        s.flag[i] = 0;
        if (lin_bnd_tighten(&s, i, &tch)) break;
        if (tch) changed = 1;
      }
    }
    if (has_inc) bnds_from_obj(&s, inc_ub, &changed);
    sets[2 * *nsweeps] = s.set[0];
    sets[2 * *nsweeps + 1] = s.set[1];
    ++*nsweeps;
    /* tightenInts_, then checkBounds_: every column, or the set's */
    for (int j = 0; j < P->n; ++j) {
      if (!is_int(P->vtype[j]) || (skip && !in_set(&s, j))) continue;
      double l = lb[j], u = ub[j];
      if (l > -INFTY && fabs(l - floor(l + 0.5)) > INT_TOL) {
        change_bflag(&s, j);
        lb[j] = ceil(l);
        s.nmods++;
        changed = 1;
      }
      if (u < INFTY && fabs(u - floor(u + 0.5)) > INT_TOL) {
        ub[j] = floor(u);
        change_bflag(&s, j);
        s.nmods++;
        changed = 1;
      }
    }
    for (int j = 0; j < P->n && !infeas; ++j)
      if ((!skip || in_set(&s, j)) && lb[j] > ub[j] + E_TOL) infeas = 1;
    if (P->cons_bad) infeas = 1;
    s.set[0] = s.set[1] = 0;
  }
  *nmods_out = s.nmods;
  return infeas;
}

/* sets: [B][MAX_SWEEPS][2] u64, nsweeps: [B] */
int k1_cols_model(int n, int m, const int *rowptr, const int *colidx, const double *val,
                  const double *rlo, const double *rhi, const int *colptr, const int *rowidx,
                  const int *vtype, int nobj, const int *objidx, const double *objval,
                  int cons_bad, int B, const double *lb_in, const double *ub_in, double *lb_out,
                  double *ub_out, int has_inc, double inc_ub, const int *clean_col, int skip,
                  int *infeas, int *nmods, uint64_t *sets, int *nsweeps)
{
  prob P;
  if (n > 128) return -1;
  P.n = n; P.m = m; P.nobj = nobj; P.cons_bad = cons_bad; P.rowptr = rowptr; P.colidx = colidx;
  P.colptr = colptr; P.rowidx = rowidx; P.vtype = vtype; P.objidx = objidx; P.val = val;
  P.rlo = rlo; P.rhi = rhi; P.objval = objval;
  unsigned char *flag = (unsigned char *) malloc((size_t) (m > 0 ? m : 1));
  for (int b = 0; b < B; ++b) {
    size_t o = (size_t) b * (size_t) n;
    memcpy(lb_out + o, lb_in + o, (size_t) n * sizeof(double));
    memcpy(ub_out + o, ub_in + o, (size_t) n * sizeof(double));
    infeas[b] = fbbt_node(&P, lb_out + o, ub_out + o, has_inc, inc_ub, flag, clean_col[b], skip,
                          nmods + b, sets + (size_t) b * MAX_SWEEPS * 2, nsweeps + b);
  }
  free(flag);
  return 0;
}
