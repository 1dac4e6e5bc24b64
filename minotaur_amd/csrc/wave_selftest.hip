// One-wave self-test of the wave.h reductions (tests/test_wave_reduce_gpu.py):
// one wave of a block runs every helper on 64 doubles and 64 ints and stores,
// per lane, what the helper leaves in that lane.
#include <hip/hip_runtime.h>

#include "mgpu.h"
#include "wave.h"

namespace mgpu {

// Rows of the outputs (out_d and out_i are [MGPU_WAVE_SELFTEST_ROWS][64]; a helper
// that has no double / no int result leaves its row zero).
enum {
  kStSumSym = 0,      // wave_sum_sym: d
  kStMax = 1,         // wave_max_dpp: d
  kStMin = 2,         // wave_min_dpp: d
  kStArgmaxLane = 3,  // wave_argmax_lane: d = the maximum, i = its lane
  kStArgmaxIdx = 4,   // wave_argmax_idx: d, i
  kStArgmaxDpp = 5,   // wave_argmax_dpp: d, i
  kStMinI32 = 6,      // wave_min_i32_dpp: i
};

__global__ void wave_selftest_kernel(const double *__restrict__ in_d, const int *__restrict__ in_i,
                                     int wave, double *__restrict__ out_d,
                                     int *__restrict__ out_i) {
  if ((int)(threadIdx.x >> 6) != wave) return;  // wave uniform: the whole wave stays or leaves
  const int lane = threadIdx.x & 63;
  const double x = in_d[lane];
  const int k = in_i[lane];
  out_d[kStSumSym * 64 + lane] = wave_sum_sym(x);
  out_d[kStMax * 64 + lane] = wave_max_dpp(x);
  out_d[kStMin * 64 + lane] = wave_min_dpp(x);
  {
    double v = x;
    const int r = wave_argmax_lane(v);
    out_d[kStArgmaxLane * 64 + lane] = v;
    out_i[kStArgmaxLane * 64 + lane] = r;
  }
  {
    double v = x;
    int i = k;
    wave_argmax_idx(v, i);
    out_d[kStArgmaxIdx * 64 + lane] = v;
    out_i[kStArgmaxIdx * 64 + lane] = i;
  }
  {
    double v = x;
    int i = k;
    wave_argmax_dpp(v, i);
    out_d[kStArgmaxDpp * 64 + lane] = v;
    out_i[kStArgmaxDpp * 64 + lane] = i;
  }
  out_i[kStMinI32 * 64 + lane] = wave_min_i32_dpp(k);
}

}  // namespace mgpu

extern "C" int mgpu_wave_selftest(int device, int block_threads, int wave, const double *in_d,
                                  const int32_t *in_i, double *out_d, int32_t *out_i) {
  if (!in_d || !in_i || !out_d || !out_i) return MGPU_ERR_ARG;
  if (block_threads < 64 || block_threads > 1024 || block_threads % 64 != 0) return MGPU_ERR_ARG;
  if (wave < 0 || wave >= block_threads / 64) return MGPU_ERR_ARG;
  constexpr int kRows = MGPU_WAVE_SELFTEST_ROWS;
  if (hipSetDevice(device) != hipSuccess) return MGPU_ERR_HIP;
  double *d_in = nullptr, *d_out = nullptr;
  int *i_in = nullptr, *i_out = nullptr;
  int rc = MGPU_ERR_HIP;
  if (hipMalloc(&d_in, 64 * sizeof(double)) == hipSuccess &&
      hipMalloc(&i_in, 64 * sizeof(int)) == hipSuccess &&
      hipMalloc(&d_out, kRows * 64 * sizeof(double)) == hipSuccess &&
      hipMalloc(&i_out, kRows * 64 * sizeof(int)) == hipSuccess &&
      hipMemcpy(d_in, in_d, 64 * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(i_in, in_i, 64 * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
      hipMemset(d_out, 0, kRows * 64 * sizeof(double)) == hipSuccess &&
      hipMemset(i_out, 0, kRows * 64 * sizeof(int)) == hipSuccess) {
    hipLaunchKernelGGL(mgpu::wave_selftest_kernel, dim3(1), dim3(block_threads), 0, 0, d_in, i_in,
                       wave, d_out, i_out);
    if (hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
        hipMemcpy(out_d, d_out, kRows * 64 * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(out_i, i_out, kRows * 64 * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess)
      rc = MGPU_OK;
  }
  (void)hipFree(d_in);
  (void)hipFree(i_in);
  (void)hipFree(d_out);
  (void)hipFree(i_out);
  return rc;
}
