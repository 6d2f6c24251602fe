// rollout_trace.hip -- replay of CHOSEN rollouts of a finished solve with everything a rollout kernel throws away: the state
// before every update, the clamped controls, every step's cost, the running mean and the step whose cost first saw the crash
// flag (mppi_trace_rollouts).  A handful of rollouts, so a latency kernel, not a throughput one:
//
//   network model: ONE WAVEFRONT PER ROLLOUT, one lane per neuron.  Lane j owns neurons j, j + 64, j + 128 and j + 192 of a layer
//   (one accumulation chain up to width 64, four at width 256); every neuron keeps the chain of nn_forward_valu
//   (rollout_valu.hip): tmp = 0, k ascending tmp = fmaf(W[j][k], act[k], tmp), then tanh_bias(tmp, b[j] * kTanhScale) on a
//   hidden layer and tmp + b[j] on the output layer -- the reference's order, so the costs are those of every order-exact
//   rollout form bit for bit.  Activations go from layer to layer through the wave's own LDS tile and come back as broadcast
//   reads, four k per ds_read_b128.  Weights come from a k-major image (pack_trace_weights: every W transposed, so that the 64
//   lanes read 256 contiguous bytes per k): from LDS where image and tiles fit kTraceLdsLimit, else from global memory; either
//   way kTraceAhead k steps are requested while the chunk before them is multiplied.  Any layer list mppi_create accepts
//   (widths up to 256, MPPI_MAX_LAYERS entries, 6-4 without a hidden layer) is a kernel argument, not a template.
//   The rest of the step is computed by all 64 lanes alike, with the device functions and in the order of rollout_valu_kernel.
//   kTraceWaves rollouts share a workgroup and its image.
//
//   basis-function model: one lane per traced rollout, the step of rollout_bf_kernel (bf_device.hpp).
//
// The controls are the solve's applied controls [T][K] (what the rollout kernels leave in place of the noise); the control
// cost is NOT computed (du = eps nu cannot be had back from them bit for bit): the ABI refuses the cost outputs where a control
// cost is on, and cost_finish<false> is the term's exact +0 everywhere else.
#include <atomic>

#include "../../include/mppi_hip.h"
#include "bf_device.hpp"
#include "mppi_kernels.hpp"

namespace mppi {

constexpr int kTraceWaves = 4;          // rollouts (wavefronts) per workgroup of the network kernel
constexpr int kTraceMaxWidth = 256;     // mppi_create's limit
constexpr int kTraceAhead = 8;          // k steps of weights in flight
constexpr int kTraceTileFloats = 2 * kTraceMaxWidth;                   // a wave's two activation tiles
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

// One layer for the wave: C chains per lane (neurons lane + 64 c), Wt the layer's k-major weights [nin][nout], b its biases.
// A lane past the layer's width walks the last neuron's weights and stores nothing.
template <int C>
__device__ __forceinline__ void trace_layer(const float *Wt, const float *b, int nin, int nout, bool hidden, const float *cur,
                                            float *nxt, int lane)
{
  int jj[C];
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; c++) {
    jj[c] = min(lane + 64 * c, nout - 1);
    acc[c] = 0.0f;
  }
  const int full = nin & ~(kTraceAhead - 1);
  float w[kTraceAhead][C];
  if (full > 0) {
#pragma unroll
    for (int u = 0; u < kTraceAhead; u++)
#pragma unroll
      for (int c = 0; c < C; c++) w[u][c] = Wt[u * nout + jj[c]];
  }
  for (int k0 = 0; k0 < full; k0 += kTraceAhead) {
    float wc[kTraceAhead][C];
#pragma unroll
    for (int u = 0; u < kTraceAhead; u++)
#pragma unroll
      for (int c = 0; c < C; c++) wc[u][c] = w[u][c];
    if (k0 + kTraceAhead < full) {  // the next chunk, requested before this one is multiplied
      const float *Wn = Wt + (size_t)(k0 + kTraceAhead) * nout;
#pragma unroll
      for (int u = 0; u < kTraceAhead; u++)
#pragma unroll
        for (int c = 0; c < C; c++) w[u][c] = Wn[u * nout + jj[c]];
    }
    float x[kTraceAhead];
#pragma unroll
    for (int q = 0; q < kTraceAhead / 4; q++) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(cur + k0 + 4 * q);  // broadcast: every lane the same address
      x[4 * q] = v[0]; x[4 * q + 1] = v[1]; x[4 * q + 2] = v[2]; x[4 * q + 3] = v[3];
    }
#pragma unroll
    for (int u = 0; u < kTraceAhead; u++)
#pragma unroll
      for (int c = 0; c < C; c++) acc[c] = fmaf(wc[u][c], x[u], acc[c]);
  }
  for (int k = full; k < nin; k++) {  // the ragged end, one k at a time (no padded multiply-add: the chain is the reference's)
    const float x = cur[k];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = fmaf(Wt[k * nout + jj[c]], x, acc[c]);
  }
#pragma unroll
  for (int c = 0; c < C; c++) {
    const float bj = b[jj[c]];
    const float y = hidden ? tanh_bias(acc[c], bj * kTanhScale) : acc[c] + bj;
    if (lane + 64 * c < nout) nxt[lane + 64 * c] = y;
  }
}

// what one lane stored to the wave's tile is what every lane of the wave reads next
__device__ __forceinline__ void trace_tile_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool LDS_IMG>
__global__ __launch_bounds__(64 * kTraceWaves) void rollout_trace_kernel(const TraceArgs a, const NetDesc net)
{
  extern __shared__ __attribute__((aligned(16))) float trace_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (LDS_IMG) {
    float *img_s = trace_lds + kTraceWaves * kTraceTileFloats;
    for (int i = threadIdx.x; i < net.num_params; i += 64 * kTraceWaves) img_s[i] = a.wimg[i];
    __syncthreads();
  }
  const int slot = blockIdx.x * kTraceWaves + wave;
  if (slot >= a.n) return;  // whole waves, behind the group's only barrier
  const float *img = LDS_IMG ? trace_lds + kTraceWaves * kTraceTileFloats : a.wimg;
  float *tile0 = trace_lds + wave * kTraceTileFloats;
  float *tile1 = tile0 + kTraceMaxWidth;
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
    trace_tile_sync();
    float *cur = tile0, *nxt = tile1;
    int off = 0;
    for (int l = 0; l + 1 < net.n_layers; l++) {
      const int nin = net.layers[l], nout = net.layers[l + 1];
      const float *Wt = img + off, *b = Wt + nin * nout;
      const bool hidden = l + 2 < net.n_layers;
      const int chains = (nout + 63) >> 6;
      if (chains == 1) trace_layer<1>(Wt, b, nin, nout, hidden, cur, nxt, lane);
      else if (chains == 2) trace_layer<2>(Wt, b, nin, nout, hidden, cur, nxt, lane);
      else if (chains == 3) trace_layer<3>(Wt, b, nin, nout, hidden, cur, nxt, lane);
      else trace_layer<4>(Wt, b, nin, nout, hidden, cur, nxt, lane);
      trace_tile_sync();
      off += nin * nout + nout;
      float *sw = cur; cur = nxt; nxt = sw;
    }
    const f32x4 d = *reinterpret_cast<const f32x4 *>(cur);
    sd[3] = d[0]; sd[4] = d[1]; sd[5] = d[2]; sd[6] = d[3];
    trace_tile_sync();  // the next step's inputs go to tile0, which may be the tile just read
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
  return kTraceTilesBytes + sizeof(float) * (size_t)net.num_params <= kTraceLdsLimit;
}

hipError_t launch_rollout_trace(const NetDesc &net, const TraceArgs &a, hipStream_t stream)
{
  if (a.n <= 0) return hipSuccess;
  if (net.n_layers < 2 || net.n_layers > MPPI_MAX_LAYERS || net.max_width > kTraceMaxWidth) return hipErrorInvalidValue;
  const dim3 grid((a.n + kTraceWaves - 1) / kTraceWaves), block(64 * kTraceWaves);
  if (trace_image_in_lds(net)) {
    // the kernel's dynamic-LDS ceiling, once per device
    static std::atomic<bool> raised[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !raised[dev].load(std::memory_order_acquire)) {
      e = hipFuncSetAttribute(reinterpret_cast<const void *>(rollout_trace_kernel<true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTraceLdsLimit);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < 64) raised[dev].store(true, std::memory_order_release);
    }
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
