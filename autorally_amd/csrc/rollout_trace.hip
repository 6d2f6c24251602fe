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
//   a fleet (mppi_trace_rollouts_batch): the two bodies again, behind a head that reads the member's argument block -- and, for the
//   network model, its layer list and image-in-LDS flag -- from an array in device memory (rollout_trace_fleet_kernel,
//   rollout_trace_fleet_bf_kernel), and in front of them trace_select_fleet_kernel, which chooses every member's best n on the device.
//
// The controls are the solve's applied controls [T][K] (what the rollout kernels leave in place of the noise); the control
// cost is NOT computed (du = eps nu cannot be had back from them bit for bit): the ABI refuses the cost outputs where a control
// cost is on, and cost_finish<false> is the term's exact +0 everywhere else.
#include "../../include/mppi_hip.h"
#include "bf_device.hpp"
#include "wave_net.hpp"

#include <algorithm>

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

// one traced rollout of the network model for its wave: img = the k-major image in LDS or in global memory (the caller has one call
// for each, so that the weights are read with LDS or global instructions), tile0 / tile1 = the wave's two activation tiles
__device__ __forceinline__ void trace_net_rollout(const TraceArgs &a, const NetDesc &net, const float *img, float *tile0, float *tile1,
                                                  int slot, int lane)
{
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

  // trace_net_rollout's statements, kept in the kernel's own text: called from here the function costs this kernel two more scalar
  // registers parked in vector lanes (profiles/r30_a_trace_fleet_isa.txt); as written the kernel is instruction for instruction what it was
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

// the traced rollouts of one workgroup of the basis-function model, one lane each: W[4][25] staged transposed into W_s first
__device__ __forceinline__ void trace_bf_group(const TraceArgs &a, float *W_s)
{
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

__global__ __launch_bounds__(kBfLanes) void rollout_trace_bf_kernel(const TraceArgs a)
{
  __shared__ __attribute__((aligned(16))) float W_s[4 * kNumBfs];  // transposed: [25][4]
  trace_bf_group(a, W_s);
}

// ---- a fleet's traces in one launch (mppi_trace_rollouts_batch) ----
// Grid (workgroups of the member with the most rollouts, members); workgroup (x, y) runs workgroup x of inst[y], an array of
// argument blocks in DEVICE memory (rollout_fleet16_kernel's head: the index is workgroup-uniform and the array read-only, so the
// block arrives in scalar registers; every pointer it holds is loaded as a global one).  A workgroup that holds no slot of its
// member leaves before it touches LDS and before the barrier.  The body is the single kernels', unchanged.
__device__ __forceinline__ TraceArgs trace_fleet_args(const TraceFleetArgs &A)
{
  TraceArgs a = A.a;
  a.V = load_global_ptr(A.a.V);
  a.ks = load_global_ptr(A.a.ks);
  a.wimg = load_global_ptr(A.a.wimg);
  a.inv_t = load_global_ptr(A.a.inv_t);
  a.states = load_global_ptr(A.a.states);
  a.controls = load_global_ptr(A.a.controls);
  a.step_costs = load_global_ptr(A.a.step_costs);
  a.costs = load_global_ptr(A.a.costs);
  a.first_crash = load_global_ptr(A.a.first_crash);
  a.cost.map = load_global_ptr(A.a.cost.map);
  return a;
}

__global__ __launch_bounds__(64 * kTraceWaves) void rollout_trace_fleet_kernel(const TraceFleetArgs *__restrict__ inst)
{
  extern __shared__ __attribute__((aligned(16))) float trace_fleet_lds[];
  const TraceFleetArgs &A = inst[blockIdx.y];  // workgroup-uniform, read-only: scalar loads
  if ((int)blockIdx.x * kTraceWaves >= A.a.n) return;  // no slot of this member: no LDS access, no barrier
  const TraceArgs a = trace_fleet_args(A);
  const NetDesc &net = A.net;  // the layer list is the member's data
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = blockIdx.x * kTraceWaves + wave;
  float *tile0 = trace_fleet_lds + wave * kTraceTileFloats;
  float *const img_lds = trace_fleet_lds + kTraceWaves * kTraceTileFloats;
  if (A.img_lds) {  // one call per image source: LDS or global instructions, no flat ones
    wave_net_stage_image(img_lds, a.wimg, net.num_params, 64 * kTraceWaves);
    __syncthreads();
    if (slot >= a.n) return;  // whole waves, behind the group's only barrier
    trace_net_rollout(a, net, img_lds, tile0, tile0 + kWaveNetMaxWidth, slot, lane);
  } else {
    if (slot >= a.n) return;
    trace_net_rollout(a, net, a.wimg, tile0, tile0 + kWaveNetMaxWidth, slot, lane);
  }
}

__global__ __launch_bounds__(kBfLanes) void rollout_trace_fleet_bf_kernel(const TraceFleetArgs *__restrict__ inst)
{
  __shared__ __attribute__((aligned(16))) float W_s[4 * kNumBfs];  // transposed: [25][4]
  const TraceFleetArgs &A = inst[blockIdx.y];
  if ((int)blockIdx.x * kBfLanes >= A.a.n) return;
  const TraceArgs a = trace_fleet_args(A);
  trace_bf_group(a, W_s);
}

// The members' "best n" chosen on the device, in front of the trace kernels on the same stream: grid (blocks of the member with
// the most rollouts, members).  Index r of a member is the rollout of rank r in mppi_top_rollouts' TOTAL order -- a number before
// a NaN, then the larger weight, then the lower index -- so the result is unique: every thread owns one rollout k, counts over
// all K weights (staged through LDS in tiles, read as broadcasts) how many precede it, and stores k at that rank where the rank
// is below the member's count.  No atomics, no order of arrival: deterministic.  Any K; a member with explicit indices (w == nullptr)
// has them already.
constexpr int kSelThreads = 256, kSelTile = 1024;

__global__ __launch_bounds__(kSelThreads) void trace_select_fleet_kernel(const TraceSelectArgs *__restrict__ inst)
{
  __shared__ __attribute__((aligned(16))) float tile[kSelTile];
  const TraceSelectArgs &A = inst[blockIdx.y];
  const int K = A.K, n = A.n;
  const float *w = load_global_ptr(A.w);
  if (w == nullptr || n <= 0 || (int)blockIdx.x * kSelThreads >= K) return;  // workgroup-uniform, before the barriers
  int *ks = load_global_ptr(A.ks);
  int *ks_out = load_global_ptr(A.ks_out);
  const int k = blockIdx.x * kSelThreads + threadIdx.x;
  const bool mine = k < K;
  const float wk = mine ? w[k] : 0.0f;
  const bool nk = wk != wk;
  int rank = 0;
  for (int j0 = 0; j0 < K; j0 += kSelTile) {
    const int m = min(kSelTile, K - j0), m4 = (m + 3) & ~3;
    __syncthreads();  // the tile before this one has been read
    // behind the last weight: NaN under an index >= K, which precedes nothing
    for (int i = threadIdx.x; i < m4; i += kSelThreads) tile[i] = (i < m) ? w[j0 + i] : __builtin_nanf("");
    __syncthreads();
    for (int i = 0; i < m4; i += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(tile + i);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const float wj = v[q];
        const int j = j0 + i + q;
        const bool nj = wj != wj;
        const bool before = nk ? (!nj || j < k) : (!nj && (wj > wk || (wj == wk && j < k)));
        rank += before ? 1 : 0;
      }
    }
  }
  if (mine && rank < n) {
    ks[rank] = k;
    if (ks_out) ks_out[rank] = k;
  }
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

hipError_t launch_trace_select_fleet(const TraceSelectArgs *h_inst, const TraceSelectArgs *d_inst, int n, hipStream_t stream)
{
  if (!h_inst || !d_inst || n < 1 || n > kMaxFleet) return hipErrorInvalidValue;
  int kmax = 0;
  for (int i = 0; i < n; i++) {
    const TraceSelectArgs &s = h_inst[i];
    if (!s.w || s.n <= 0) continue;
    if (!s.ks || s.n > s.K) return hipErrorInvalidValue;
    kmax = std::max(kmax, s.K);
  }
  if (kmax == 0) return hipSuccess;  // every member brought its indices
  hipLaunchKernelGGL(trace_select_fleet_kernel, dim3((kmax + kSelThreads - 1) / kSelThreads, n), dim3(kSelThreads), 0, stream, d_inst);
  return hipGetLastError();
}

// h_inst: the n argument blocks on the host (counts, layer lists and image flags are read there); d_inst: the same blocks in
// device memory, complete once `stream` reaches the launch
hipError_t launch_rollout_trace_fleet(const TraceFleetArgs *h_inst, const TraceFleetArgs *d_inst, int n, hipStream_t stream)
{
  if (!h_inst || !d_inst || n < 1 || n > kMaxFleet) return hipErrorInvalidValue;
  int nmax = 0;
  size_t lds = kTraceTilesBytes;
  for (int i = 0; i < n; i++) {
    const TraceFleetArgs &m = h_inst[i];
    if (m.a.n < 0 || m.a.n > m.a.K || m.a.T < 1 || !wave_net_valid(m.net)) return hipErrorInvalidValue;
    if (m.img_lds) {
      if (!trace_image_in_lds(m.net)) return hipErrorInvalidValue;
      lds = std::max(lds, kTraceTilesBytes + sizeof(float) * (size_t)m.net.num_params);
    }
    nmax = std::max(nmax, m.a.n);
  }
  if (nmax == 0) return hipSuccess;
  if (hipError_t e = raise_lds_limit_once<rollout_trace_fleet_kernel>(kTraceLdsLimit); e != hipSuccess) return e;
  hipLaunchKernelGGL(rollout_trace_fleet_kernel, dim3((nmax + kTraceWaves - 1) / kTraceWaves, n), dim3(64 * kTraceWaves), lds, stream, d_inst);
  return hipGetLastError();
}

hipError_t launch_rollout_trace_fleet_bf(const TraceFleetArgs *h_inst, const TraceFleetArgs *d_inst, int n, hipStream_t stream)
{
  if (!h_inst || !d_inst || n < 1 || n > kMaxFleet) return hipErrorInvalidValue;
  int nmax = 0;
  for (int i = 0; i < n; i++) {
    if (h_inst[i].a.n < 0 || h_inst[i].a.n > h_inst[i].a.K || h_inst[i].a.T < 1) return hipErrorInvalidValue;
    nmax = std::max(nmax, h_inst[i].a.n);
  }
  if (nmax == 0) return hipSuccess;
  hipLaunchKernelGGL(rollout_trace_fleet_bf_kernel, dim3((nmax + kBfLanes - 1) / kBfLanes, n), dim3(kBfLanes), 0, stream, d_inst);
  return hipGetLastError();
}

}  // namespace mppi
