// Node migration between ranks of the node-sharded spatial tree (SURVEY §8 e),
// gfx950.  MpiBranchAndBound::LoadBalance_ (src/base/MpiBranchAndBound.cpp:
// 78-195) serialises every node it hands to another rank and sends it with
// one MPI_Send per node; the receiving rank's NodeIncRelaxer replays the
// node's modifications on its own relaxation.  A node of the batched glob
// tree is more than its box: K2 rewrites the secant / McCormick rows from
// the PARENT's row state, the separation loop fills the square's next free
// tangent slot, K3R refactors the parent's optimal basis (warm 1) and
// relstronger's updateAfterSolve reads the branching that made the node.  So
// all of it crosses, packed on the device into one f64 row per node, every
// field exact:
//     row t = [ lb (nv) | ub (nv) | rows (R) | tan (T) | node bound | depth ]
//     warm 1:        + [ has_basis | head (m) | statuses packed ]
//     brancher >= 1: + [ var | isint | act | dd | ud | plb ]
// Integers are stored as doubles; the basis statuses 2 bits each, 16 per
// double (ceil((nv + m) / 16) doubles), as bnb_pack does.  A row with
// has_basis 0 carries zeros for head and statuses and leaves its slot without
// a basis (pws_ok 0: the node LP starts from the slack basis, as the root's).
// The branching records are host state per pool slot (GlobState::BrInfo), so
// they pass through a staging array [k][kMigStage] that the host fills
// (pack) or reads (unpack) with one copy per exchange; unpack also leaves the
// node bound and depth there for the host's NodeHeap.
// Two kernels, one wave per node, four per 256-thread block, lanes striding
// the arrays (coalesced), no LDS, no atomics:
//   glob_pack   : pool slot slots[t] -> row t;
//   glob_unpack : row t -> pool slot slots[t].
// The depth-first stack closes the gaps exported nodes leave with
// bnb_migrate.hip's generic row move (launch_bnb_move_rows).
#include "glob_internal.h"

namespace mgpu {
namespace {

__global__ __launch_bounds__(256) void glob_pack(GlobMigIO io) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= io.k) return;
  const int nv = io.nv, R = io.R, T = io.T;
  const size_t s = (size_t)io.slots[t];
  double *row = io.rows + (size_t)t * io.W;
  for (int j = lane; j < nv; j += 64) {
    row[j] = io.plb[s * nv + j];
    row[nv + j] = io.pub[s * nv + j];
  }
  double *w = row + 2 * nv;
  for (int j = lane; j < R; j += 64) w[j] = io.prows[s * R + j];
  w += R;
  for (int j = lane; j < T; j += 64) w[j] = io.ptan[s * T + j];
  w += T;
  if (lane == 0) {
    w[0] = io.pnlb[s];
    w[1] = (double)io.pdepth[s];
  }
  w += 2;
  if (io.warm) {   // the parent's optimal basis travels with the node
    const int m = io.m, N = io.N;
    const bool ok = io.pws_ok[s] != 0;
    if (lane == 0) w[0] = ok ? 1.0 : 0.0;
    for (int j = lane; j < m; j += 64) w[1 + j] = ok ? (double)io.pws_head[s * m + j] : 0.0;
    const int nq = (N + 15) / 16;
    for (int q = lane; q < nq; q += 64) {
      uint32_t bits = 0;
      if (ok)
        for (int i = 0; i < 16 && q * 16 + i < N; ++i)
          bits |= (uint32_t)(io.pws_st[s * N + q * 16 + i] & 3) << (2 * i);
      w[1 + m + q] = (double)bits;
    }
    w += 1 + m + nq;
  }
  if (io.br && lane < 6) w[lane] = io.stage[(size_t)t * kMigStage + 2 + lane];
}

__global__ __launch_bounds__(256) void glob_unpack(GlobMigIO io) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= io.k) return;
  const int nv = io.nv, R = io.R, T = io.T;
  const size_t s = (size_t)io.slots[t];
  const double *row = io.rows + (size_t)t * io.W;
  for (int j = lane; j < nv; j += 64) {
    io.plb[s * nv + j] = row[j];
    io.pub[s * nv + j] = row[nv + j];
  }
  const double *w = row + 2 * nv;
  for (int j = lane; j < R; j += 64) io.prows[s * R + j] = w[j];
  w += R;
  for (int j = lane; j < T; j += 64) io.ptan[s * T + j] = w[j];
  w += T;
  double *stg = io.stage + (size_t)t * kMigStage;
  if (lane == 0) {
    io.pnlb[s] = w[0];
    io.pdepth[s] = (int32_t)w[1];
  }
  if (lane < 2) stg[lane] = w[lane];
  w += 2;
  if (io.warm) {
    const int m = io.m, N = io.N;
    const bool ok = w[0] != 0.0;
    if (lane == 0) io.pws_ok[s] = ok ? 1 : 0;
    if (ok) {
      for (int j = lane; j < m; j += 64) io.pws_head[s * m + j] = (int32_t)w[1 + j];
      for (int j = lane; j < N; j += 64) {
        const uint32_t bits = (uint32_t)w[1 + m + j / 16];
        io.pws_st[s * N + j] = (int8_t)((bits >> (2 * (j % 16))) & 3u);
      }
    }
    w += 1 + m + (N + 15) / 16;
  }
  if (lane < 6) stg[2 + lane] = io.br ? w[lane] : (lane == 0 ? -1.0 : 0.0);
}

}  // namespace

hipError_t launch_glob_mig_pack(const GlobMigIO &io, hipStream_t stream) {
  if (io.k <= 0) return hipSuccess;
  hipLaunchKernelGGL(glob_pack, dim3((io.k + 3) / 4), dim3(256), 0, stream, io);
  return hipGetLastError();
}

hipError_t launch_glob_mig_unpack(const GlobMigIO &io, hipStream_t stream) {
  if (io.k <= 0) return hipSuccess;
  hipLaunchKernelGGL(glob_unpack, dim3((io.k + 3) / 4), dim3(256), 0, stream, io);
  return hipGetLastError();
}

}  // namespace mgpu
