// wave_net.hpp -- the per-wave network forward: ONE WAVEFRONT evaluates one network, one lane per neuron.  Lane j owns neurons j,
// j + 64, j + 128 and j + 192 of a layer (one accumulation chain up to width 64, four at width 256), every chain k ascending from
// 0.  Activations go from layer to layer through the wave's two LDS tiles and come back as broadcast reads, four k per
// ds_read_b128.  Weights come from the k-major image (Image::Trace, pack_trace_weights: every W transposed, so that the 64 lanes
// read 256 contiguous bytes per k), in LDS or in global memory; kWaveNetAhead k steps are requested while the chunk before them
// is multiplied.  Any layer list mppi_create accepts is data.
//
// Used by rollout_trace.hip (the traced rollouts), ddp_fleet.hip (through ddp_f), nominal_fleet.hip and nominal_gains_fleet.hip.  What differs between
// them is an arithmetic policy: how a neuron's sum takes one product, and what follows the sum.  The library is compiled
// -ffp-contract=off, so a policy's text is its arithmetic: an fmaf is one rounding, a multiply and an add are two.
#pragma once
#include "../../include/mppi_hip.h"
#include "mppi_kernels.hpp"
#include "tanhf_scalar.hpp"

namespace mppi {

constexpr int kWaveNetAhead = 8;       // k steps of weights in flight
constexpr int kWaveNetMaxWidth = 256;  // mppi_create's limit; a wave's activation tile

// the rollout kernels' neuron (nn_forward_valu, rollout_valu.hip): fmaf chain, tanh_bias on a hidden layer
struct WaveArithRollout {
  static __device__ __forceinline__ float mac(float acc, float w, float x) { return fmaf(w, x, acc); }
  static __device__ __forceinline__ float finish(float acc, float bias, bool hidden)
  {
    return hidden ? tanh_bias(acc, bias * kTanhScale) : acc + bias;
  }
};
// the host replay's neuron (HostNetFma::forward, host_net.hpp): fmaf chain, the bias added afterwards, tanhf on a hidden layer
struct WaveArithHostFma {
  static __device__ __forceinline__ float mac(float acc, float w, float x) { return fmaf(w, x, acc); }
  static __device__ __forceinline__ float finish(float acc, float bias, bool hidden)
  {
    const float y = acc + bias;
    return hidden ? tanhf_scalar(y) : y;
  }
};
// the DDP pass's neuron (HostNet::forward, ddp_feedback.cpp): a SEPARATE multiply and add, the bias added afterwards, tanhf on a
// hidden layer
struct WaveArithHostMulAdd {
  static __device__ __forceinline__ float mac(float acc, float w, float x) { return acc + w * x; }
  static __device__ __forceinline__ float finish(float acc, float bias, bool hidden)
  {
    const float y = acc + bias;
    return hidden ? tanhf_scalar(y) : y;
  }
};

// what one lane stored to the wave's tile is what every lane of the wave reads next
__device__ __forceinline__ void wave_tile_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One layer for the wave: C chains per lane (neurons lane + 64 c), Wt the layer's k-major weights [nin][nout], b its biases.
// th: where a hidden layer's values are kept as well (the DDP pass's Jacobian; nullptr: not kept).  A lane past the layer's width
// walks the last neuron's weights and stores nothing.
template <int C, class Arith>
__device__ __forceinline__ void wave_layer(const float *Wt, const float *b, int nin, int nout, bool hidden, const float *cur,
                                           float *nxt, float *th, int lane)
{
  int jj[C];
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; c++) {
    jj[c] = min(lane + 64 * c, nout - 1);
    acc[c] = 0.0f;
  }
  const int full = nin & ~(kWaveNetAhead - 1);
  float w[kWaveNetAhead][C];
  if (full > 0) {
#pragma unroll
    for (int u = 0; u < kWaveNetAhead; u++)
#pragma unroll
      for (int c = 0; c < C; c++) w[u][c] = Wt[u * nout + jj[c]];
  }
  for (int k0 = 0; k0 < full; k0 += kWaveNetAhead) {
    float wc[kWaveNetAhead][C];
#pragma unroll
    for (int u = 0; u < kWaveNetAhead; u++)
#pragma unroll
      for (int c = 0; c < C; c++) wc[u][c] = w[u][c];
    if (k0 + kWaveNetAhead < full) {  // the next chunk, requested before this one is multiplied
      const float *Wn = Wt + (size_t)(k0 + kWaveNetAhead) * nout;
#pragma unroll
      for (int u = 0; u < kWaveNetAhead; u++)
#pragma unroll
        for (int c = 0; c < C; c++) w[u][c] = Wn[u * nout + jj[c]];
    }
    float x[kWaveNetAhead];
#pragma unroll
    for (int q = 0; q < kWaveNetAhead / 4; q++) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(cur + k0 + 4 * q);  // broadcast: every lane the same address
      x[4 * q] = v[0]; x[4 * q + 1] = v[1]; x[4 * q + 2] = v[2]; x[4 * q + 3] = v[3];
    }
#pragma unroll
    for (int u = 0; u < kWaveNetAhead; u++)
#pragma unroll
      for (int c = 0; c < C; c++) acc[c] = Arith::mac(acc[c], wc[u][c], x[u]);
  }
  for (int k = full; k < nin; k++) {  // the ragged end, one k at a time (no padded multiply-add: the chain is the reference's)
    const float x = cur[k];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = Arith::mac(acc[c], Wt[k * nout + jj[c]], x);
  }
#pragma unroll
  for (int c = 0; c < C; c++) {
    const float y = Arith::finish(acc[c], b[jj[c]], hidden);
    if (lane + 64 * c < nout) {
      nxt[lane + 64 * c] = y;
      if (hidden && th) th[lane + 64 * c] = y;
    }
  }
}

// The network for the wave.  The caller has stored the six inputs to tile0 (how is the caller's: part of its instruction stream);
// img: the k-major image, in LDS or in global memory; tile0 / tile1: the wave's two tiles, kWaveNetMaxWidth floats each; th: the
// hidden layers' values [sum of hidden widths] or nullptr.  Returns the four outputs, the same in every lane.  The tiles are free
// again on return: the next inputs may go to tile0 at once.
template <class Arith>
__device__ __forceinline__ f32x4 wave_net_forward(const NetDesc &net, const float *img, float *tile0, float *tile1, float *th,
                                                  int lane)
{
  wave_tile_sync();
  float *cur = tile0, *nxt = tile1;
  int off = 0, hoff = 0;
  for (int l = 0; l + 1 < net.n_layers; l++) {
    const int nin = net.layers[l], nout = net.layers[l + 1];
    const float *Wt = img + off, *b = Wt + nin * nout;
    const bool hidden = l + 2 < net.n_layers;
    float *thl = (th && hidden) ? th + hoff : nullptr;
    const int chains = (nout + 63) >> 6;
    if (chains == 1) wave_layer<1, Arith>(Wt, b, nin, nout, hidden, cur, nxt, thl, lane);
    else if (chains == 2) wave_layer<2, Arith>(Wt, b, nin, nout, hidden, cur, nxt, thl, lane);
    else if (chains == 3) wave_layer<3, Arith>(Wt, b, nin, nout, hidden, cur, nxt, thl, lane);
    else wave_layer<4, Arith>(Wt, b, nin, nout, hidden, cur, nxt, thl, lane);
    wave_tile_sync();
    off += nin * nout + nout;
    hoff += nout;
    float *sw = cur; cur = nxt; nxt = sw;
  }
  const f32x4 d = *reinterpret_cast<const f32x4 *>(cur);
  wave_tile_sync();  // the next step's inputs go to tile0, which may be the tile just read
  return d;
}

// the workgroup's `threads` threads copy the image to LDS; the caller's barrier follows
__device__ __forceinline__ void wave_net_stage_image(float *dst, const float *src, int num_params, int threads)
{
  for (int i = threadIdx.x; i < num_params; i += threads) dst[i] = src[i];
}

// launch checks: a layer list the forward takes, and whether its image fits a kernel's LDS budget beside `fixed_floats` of tiles
inline bool wave_net_valid(const NetDesc &net)
{
  return net.n_layers >= 2 && net.n_layers <= MPPI_MAX_LAYERS && net.max_width <= kWaveNetMaxWidth;
}
inline bool wave_net_image_in_lds(const NetDesc &net, size_t fixed_floats, size_t limit_bytes)
{
  return sizeof(float) * (fixed_floats + (size_t)net.num_params) <= limit_bytes;
}

}  // namespace mppi
