// rollout_trace.hip -- replay of CHOSEN rollouts of a finished solve with everything a rollout kernel throws away: the state
// before every update, the clamped controls, every step's cost, the running mean and the step whose cost first saw the crash
// flag (mppi_trace_rollouts).  A handful of rollouts, so a latency kernel, not a throughput one:
//
//   network model: ONE WAVEFRONT PER ROLLOUT, one lane per neuron: the per-wave forward of wave_net.hpp with the rollout
//   kernels' neuron (WaveArithRollout), which keeps the chain of nn_forward_valu (rollout_valu.hip): tmp = 0, k ascending
//   tmp = fmaf(W[j][k], act[k], tmp), then tanh_bias(tmp, b[j] * kTanhScale) on a hidden layer and tmp + b[j] on the output
//   layer -- the reference's order, so the costs are those of every order-exact rollout form bit for bit.  The k-major image
//   (pack_trace_weights) is read from LDS where image and tiles fit kTraceLdsLimit, else from global memory.  Any layer list
//   mppi_create accepts (widths up to 256, MPPI_MAX_LAYERS entries, 6-4 without a hidden layer) is a kernel argument, not a
//   template.
//   The rest of the step is computed by all 64 lanes alike, with the device functions and in the order of rollout_valu_kernel.
//   kTraceWaves rollouts share a workgroup and its image.
//
//   basis-function model: one lane per traced rollout, the step of rollout_bf_kernel (bf_device.hpp).
//
// The controls are the solve's applied controls [T][K] (what the rollout kernels leave in place of the noise); the control
// cost is NOT computed (du = eps nu cannot be had back from them bit for bit): the ABI refuses the cost outputs where a control
// cost is on, and cost_finish<false> is the term's exact +0 everywhere else.
#include "../../include/mppi_hip.h"
#include "bf_device.hpp"
#include "wave_net.hpp"

namespace mppi {

constexpr int kTraceWaves = 4;          // rollouts (wavefronts) per workgroup of the network kernel
constexpr int kTraceTileFloats = 2 * kWaveNetMaxWidth;                 // a wave's two activation tiles
constexpr size_t kTraceLdsLimit = 64 * 1024;                           // tiles + image: beside a gated latency launch on the same CU
constexpr size_t kTraceTilesBytes = sizeof(float) * kTraceWaves * kTraceTileFloats;

// what one rollout's wave (network) or lane (basis functions) carries through its T steps
struct TraceRun {
  float s[kStateDim];
  float J;
  int crash, first;
};

__device__ __forceinline__ void trace_begin(const TraceArgs &a, TraceRun &r)
{
#pragma unroll
  for (int i = 0; i < kStateDim; i++) r.s[i] = a.state[i];
  r.J = 0.0f;
  r.crash = 0;
  r.first = -1;
}

// the head of step t: controls after the clamp, sin / cos of the heading, the two costmap texels (from t = 1 on)
__device__ __forceinline__ void trace_head(const TraceArgs &a, const TraceRun &r, int k, int t, float &u0, float &u1, float &spsi,
                                           float &cpsi, float &tf, float &tb)
{
  const float2 v = reinterpret_cast<const float2 *>(a.V)[(size_t)t * a.K + k];
  u0 = clampf(v.x, a.u_lo[0], a.u_hi[0]);
  u1 = clampf(v.y, a.u_lo[1], a.u_hi[1]);
  sincos_fast(r.s[2], spsi, cpsi);
  tf = 0.0f;
  tb = 0.0f;
  if (t > 0) {
    if (a.cost.affine) track_fetch<true>(a.cost, r.s, cpsi, spsi, tf, tb);
    else track_fetch<false>(a.cost, r.s, cpsi, spsi, tf, tb);
  }
}

// the rest of step t once sd is known: cost before the update, records (write: one lane per rollout), update, sticky roll flag
__device__ __forceinline__ void trace_tail(const TraceArgs &a, TraceRun &r, int slot, int t, float u0, float u1, float tf, float tb,
                                           const float (&sd)[kStateDim], bool write)
{
  float c = 0.0f;
  if (t > 0) {
    c = cost_finish<false>(a.cost, a.nu, r.s[4], r.s[5], tf, tb, u0, u1, 0.0f, 0.0f, r.crash);
    r.J = running_mean(r.J, c, t, a.inv_t[t]);
    r.first = (r.crash > 0 && r.first < 0) ? t : r.first;
  }
  if (write) {
    const size_t at = (size_t)slot * a.T + t;
    if (a.states) {
#pragma unroll
      for (int i = 0; i < kStateDim; i++) a.states[at * kStateDim + i] = r.s[i];
    }
    if (a.controls) {
      a.controls[at * 2] = u0;
      a.controls[at * 2 + 1] = u1;
    }
    if (a.step_costs) a.step_costs[at] = c;
  }
#pragma unroll
  for (int i = 0; i < kStateDim; i++) r.s[i] = fmaf(sd[i], a.dt, r.s[i]);
  r.crash |= (int)(fabsf(r.s[3]) >= kRollCrash);
}

__device__ __forceinline__ void trace_end(const TraceArgs &a, const TraceRun &r, int slot)
{
  if (a.costs) a.costs[slot] = r.J + 0.0f;
  if (a.first_crash) a.first_crash[slot] = r.first;
}

template <bool LDS_IMG>
__global__ __launch_bounds__(64 * kTraceWaves) void rollout_trace_kernel(const TraceArgs a, const NetDesc net)
{
  extern __shared__ __attribute__((aligned(16))) float trace_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (LDS_IMG) {
    wave_net_stage_image(trace_lds + kTraceWaves * kTraceTileFloats, a.wimg, net.num_params, 64 * kTraceWaves);
    __syncthreads();
  }
  const int slot = blockIdx.x * kTraceWaves + wave;
  if (slot >= a.n) return;  // whole waves, behind the group's only barrier
  const float *img = LDS_IMG ? trace_lds + kTraceWaves * kTraceTileFloats : a.wimg;
  float *tile0 = trace_lds + wave * kTraceTileFloats;
  float *tile1 = tile0 + kWaveNetMaxWidth;
  const int k = a.ks[slot];

  TraceRun r;
  trace_begin(a, r);
  for (int t = 0; t < a.T; t++) {
    float u0, u1, spsi, cpsi, tf, tb;
    trace_head(a, r, k, t, u0, u1, spsi, cpsi, tf, tb);
    float sd[kStateDim];
    sd[0] = fmaf(cpsi, r.s[4], -(spsi * r.s[5]));
    sd[1] = fmaf(spsi, r.s[4], cpsi * r.s[5]);
    sd[2] = a.negate_yaw_der ? -r.s[6] : r.s[6];
    {
      const float lo = (lane == 0) ? r.s[3] : (lane == 1) ? r.s[4] : r.s[5];
      const float hi = (lane == 3) ? r.s[6] : (lane == 4) ? u0 : u1;
      if (lane < kNetIn) tile0[lane] = (lane < 3) ? lo : hi;
    }
    const f32x4 d = wave_net_forward<WaveArithRollout>(net, img, tile0, tile1, nullptr, lane);
    sd[3] = d[0]; sd[4] = d[1]; sd[5] = d[2]; sd[6] = d[3];
    trace_tail(a, r, slot, t, u0, u1, tf, tb, sd, lane == 0);
  }
  if (lane == 0) trace_end(a, r, slot);
}

__global__ __launch_bounds__(kBfLanes) void rollout_trace_bf_kernel(const TraceArgs a)
{
  __shared__ __attribute__((aligned(16))) float W_s[4 * kNumBfs];  // transposed: [25][4]
  const int lane = threadIdx.x;
  for (int i = lane; i < 4 * kNumBfs; i += kBfLanes) W_s[(i % kNumBfs) * 4 + i / kNumBfs] = a.wimg[i];
  __syncthreads();
  const int slot = blockIdx.x * kBfLanes + lane;
  if (slot >= a.n) return;
  BfWeights Wr;
  Wr.load(W_s);
  const int k = a.ks[slot];
  TraceRun r;
  trace_begin(a, r);
  for (int t = 0; t < a.T; t++) {
    float u0, u1, spsi, cpsi, tf, tb;
    trace_head(a, r, k, t, u0, u1, spsi, cpsi, tf, tb);
    float sd[kStateDim];
    bf_state_deriv(Wr, r.s, u0, u1, cpsi, spsi, sd);
    trace_tail(a, r, slot, t, u0, u1, tf, tb, sd, true);
  }
  trace_end(a, r, slot);
}

bool trace_image_in_lds(const NetDesc &net)
{
  return wave_net_image_in_lds(net, (size_t)kTraceWaves * kTraceTileFloats, kTraceLdsLimit);
}

hipError_t launch_rollout_trace(const NetDesc &net, const TraceArgs &a, hipStream_t stream)
{
  if (a.n <= 0) return hipSuccess;
  if (!wave_net_valid(net)) return hipErrorInvalidValue;
  const dim3 grid((a.n + kTraceWaves - 1) / kTraceWaves), block(64 * kTraceWaves);
  if (trace_image_in_lds(net)) {
    if (hipError_t e = raise_lds_limit_once<rollout_trace_kernel<true>>(kTraceLdsLimit); e != hipSuccess) return e;
    const size_t lds = kTraceTilesBytes + sizeof(float) * (size_t)net.num_params;
    hipLaunchKernelGGL(rollout_trace_kernel<true>, grid, block, lds, stream, a, net);
  } else {
    hipLaunchKernelGGL(rollout_trace_kernel<false>, grid, block, kTraceTilesBytes, stream, a, net);
  }
  return hipGetLastError();
}

hipError_t launch_rollout_trace_bf(const TraceArgs &a, hipStream_t stream)
{
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(rollout_trace_bf_kernel, dim3((a.n + kBfLanes - 1) / kBfLanes), dim3(kBfLanes), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mppi
