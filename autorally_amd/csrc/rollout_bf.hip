// rollout_bf.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) with the reference's second
// dynamics family, GeneralizedLinear<CarBasisFuncs,7,2,25,CarKinematics,3>
// (PI/generalized_linear.cu:169-245, PI/car_bfs.cuh:44-120), SURVEY 8f row f3.
//
// One lane per rollout, with the work of 64 rollouts on one, two or three wavefronts of a workgroup.  The workgroups are
// bf_group.hpp's (bf1_group, bf2_group, bf3_group: device functions of (argument block, group), shared with
// rollout_fleet_bf.hip); the kernels here run group blockIdx.x of their kernel argument.  Noise comes from the stand-alone
// generator (one and two waves) or from the control wave's in-kernel generator (three waves).
#include "bf_group.hpp"

namespace mppi {

__global__ __launch_bounds__(kBfLanes) void rollout_bf_kernel(const RolloutArgs a) { bf1_group(a, (int)blockIdx.x); }

__global__ __launch_bounds__(2 * kBfLanes) void rollout_bf2_kernel(const RolloutArgs a) { bf2_group(a, (int)blockIdx.x); }

__global__ __launch_bounds__(3 * kBfLanes) void rollout_bf3_kernel(const RolloutArgs a) { bf3_group(a, (int)blockIdx.x); }

// several instances in one launch (mppi_compute_control_batch: the two controllers of path_integral_bf's control
// loop): workgroup (x, y) runs group x of instance y
template <int NB>
__global__ __launch_bounds__(3 * kBfLanes) void rollout_bf3_batch_kernel(const QuadBatchArgsT<NB> b)
{
  // the instance from the workgroup's own index, its argument block at a compile-time position (MPPI_BATCH_DISPATCH)
#define MPPI_BF_BODY(A)                                  \
  do {                                                   \
    if ((int)blockIdx.x >= (A).K / kBfLanes) return;     \
    bf3_group((A), (int)blockIdx.x);                     \
  } while (0)
  MPPI_BATCH_DISPATCH(NB, b, MPPI_BF_BODY);
#undef MPPI_BF_BODY
}

// test entry (mppi_debug_dynamics): state derivative of n independent (state, control) pairs
__global__ __launch_bounds__(kBfLanes) void dynamics_bf_kernel(const float *W, const float *states,
                                                               const float *controls, float *ders, int n)
{
  __shared__ __attribute__((aligned(16))) float W_s[4 * kNumBfs];  // transposed: [25][4]
  const int lane = threadIdx.x;
  for (int i = lane; i < 4 * kNumBfs; i += kBfLanes) W_s[(i % kNumBfs) * 4 + i / kNumBfs] = W[i];
  __syncthreads();
  const int idx = blockIdx.x * kBfLanes + lane;
  if (idx >= n) return;
  float s[kStateDim];
#pragma unroll
  for (int i = 0; i < kStateDim; i++) s[i] = states[idx * kStateDim + i];
  float spsi, cpsi;
  sincos_fast(s[2], spsi, cpsi);
  float sd[kStateDim];
  BfWeights Wr;
  Wr.load(W_s);
  bf_state_deriv(Wr, s, controls[idx * 2], controls[idx * 2 + 1], cpsi, spsi, sd);
#pragma unroll
  for (int i = 0; i < kStateDim; i++) ders[idx * kStateDim + i] = sd[i];
}

hipError_t launch_rollout_bf(const RolloutArgs &a, int waves, hipStream_t stream)
{
  if (waves == 3) MPPI_LAUNCH_ROLLOUT(rollout_bf3_kernel, dim3(a.K / kBfLanes), dim3(3 * kBfLanes), 0, stream, a);
  else if (waves == 2) MPPI_LAUNCH_ROLLOUT(rollout_bf2_kernel, dim3(a.K / kBfLanes), dim3(2 * kBfLanes), 0, stream, a);
  else MPPI_LAUNCH_ROLLOUT(rollout_bf_kernel, dim3(a.K / kBfLanes), dim3(kBfLanes), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_rollout_bf_batch(const QuadBatchArgs &b, hipStream_t stream)
{
  if (b.n < 1 || b.n > kMaxBatch) return hipErrorInvalidValue;
  int gmax = 0;
  for (int i = 0; i < b.n; i++) gmax = b.inst[i].K / kBfLanes > gmax ? b.inst[i].K / kBfLanes : gmax;
  if (b.n <= 2) hipLaunchKernelGGL(rollout_bf3_batch_kernel<2>, dim3(gmax, b.n), dim3(3 * kBfLanes), 0, stream, batch_args_prefix<2>(b));
  else hipLaunchKernelGGL(rollout_bf3_batch_kernel<4>, dim3(gmax, b.n), dim3(3 * kBfLanes), 0, stream, b);
  return hipGetLastError();
}

hipError_t launch_dynamics_bf(const float *W, const float *states, const float *controls, float *ders, int n,
                              hipStream_t stream)
{
  hipLaunchKernelGGL(dynamics_bf_kernel, dim3((n + kBfLanes - 1) / kBfLanes), dim3(kBfLanes), 0, stream, W, states,
                     controls, ders, n);
  return hipGetLastError();
}

}  // namespace mppi
