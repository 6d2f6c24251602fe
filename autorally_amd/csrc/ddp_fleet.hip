// ddp_fleet.hip -- DDP feedback gains for a whole fleet in ONE launch (mppi_compute_feedback_gains_batch): grid (n), one workgroup
// per controller, its argument block read from an array in device memory (the way rollout_fleet16_kernel reads its own).  The
// kernel restates ddp_feedback.cpp: ddp_feedback_gains for the network model operation for operation (ddp_fleet_device.hpp), so a
// handle's gains are those of its host pass up to sinf / cosf of the heading, which are the rounded double results here.
//
// A pass is three sequential recurrences of T steps and T independent Jacobians -- the latency shape:
//   A  initial rollout, wave 0: wave_net.hpp's per-wave forward (lane j owns neurons j, j + 64, j + 128, j + 192; activations through an
//      LDS tile as broadcast reads; weights from the k-major image, in LDS where it fits, else from global memory); x[t], the
//      clamped u[t], sin / cos of the heading and every hidden layer's tanh values are kept per step
//   B  the T - 1 Jacobians the backward pass reads, step t on wave t mod kDdpFleetWaves: lane = input neuron, four output chains per
//      lane, k ascending over the layer's outputs, the weights row-major (theta itself); scaled by dt, + I; the step's dL beside them
//   C  Riccati recursion, wave 0: an 8 x 8 padded tile is the wave's 64 lanes, lane (i, j) owns element (i, j) of every 7 x 7 /
//      2 x 7 product; column 7 of a tile carries the vector that goes with it (Vx beside Vxx, qx beside qxx, qu beside qux, lk
//      beside Lk), so that a vector's sum is its matrix's sum in the spare lanes
//   D  forward pass with the gains, wave 0: the wave of A; the per-step costs and their k-ascending total
// Any layer list mppi_create accepts (widths up to 256) is data.  A factorisation that is not `ok` ends the pass with status 1.
#include "../../include/mppi_hip.h"
#include "ddp_fleet_device.hpp"

namespace mppi {

__global__ __launch_bounds__(64 * kDdpFleetWaves) void ddp_fleet_kernel(const DdpFleetArgs *__restrict__ inst)
{
  extern __shared__ __attribute__((aligned(16))) float ddp_lds[];
  const DdpFleetArgs &A = inst[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  DdpFleetPtrs P;
  P.theta = load_global_ptr(A.theta);
  const float *wimg = load_global_ptr(A.wimg);
  const float *in = load_global_ptr(A.in);
  float *out = load_global_ptr(A.out);
  float *work = load_global_ptr(A.work);
  DdpFleetVals V;
  V.H = A.T; V.negate = A.negate_yaw_der;
  V.dt = A.dt;
  V.ulo0 = A.u_lo[0]; V.ulo1 = A.u_lo[1]; V.uhi0 = A.u_hi[0]; V.uhi1 = A.u_hi[1];
  V.hidden = ddp_fleet_hidden(A.net);  // the layer list stays in the argument block: read where a layer begins
  P.x0 = in; P.tx = in + 7; P.tu = in + 7 + (size_t)7 * V.H;
  ddp_fleet_lay_out(P, out, work, V.H);

  P.tile0 = ddp_lds; P.tile1 = ddp_lds + kWaveNetMaxWidth;
  float *delta = ddp_lds + kDdpActFloats + wave * kDdpDeltaFloats;
  P.img = wimg;
  if (A.img_lds) {
    float *img_s = ddp_lds + kDdpFixedFloats;
    wave_net_stage_image(img_s, wimg, A.net.num_params, 64 * kDdpFleetWaves);
    P.img = img_s;
  }
  __syncthreads();

  float xs[7];  // x[H - 1] afterwards (wave 0)
  if (wave == 0) ddp_phase_a(A, V, P, xs, lane);
  __syncthreads();  // wave 0's records (global memory) are the workgroup's
  ddp_phase_b(A, V, P, delta, wave, lane);
  __syncthreads();
  if (wave != 0) return;  // C and D are one wave's; no workgroup barrier below
  float Vlast;
  if (ddp_phase_c(A, V, P, delta, xs, Vlast, lane) != 0) return;
  ddp_phase_d(A, V, P, delta, Vlast, lane);
}

__global__ __launch_bounds__(256) void device_tanhf_kernel(const float *__restrict__ in, float *__restrict__ out, size_t n)
{
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = tanhf_scalar(in[i]);
}

bool ddp_fleet_image_in_lds(const NetDesc &net)
{
  return wave_net_image_in_lds(net, kDdpFixedFloats, kDdpLdsLimit);
}

hipError_t launch_ddp_fleet(const DdpFleetArgs *h_inst, const DdpFleetArgs *d_inst, int n, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  if (n > kMaxFleet) return hipErrorInvalidValue;
  size_t lds = sizeof(float) * (size_t)kDdpFixedFloats;
  for (int i = 0; i < n; i++) {
    const NetDesc &net = h_inst[i].net;
    if (!wave_net_valid(net) || h_inst[i].T < 2) return hipErrorInvalidValue;
    if (h_inst[i].img_lds) {
      if (!ddp_fleet_image_in_lds(net)) return hipErrorInvalidValue;
      lds = std::max(lds, sizeof(float) * ((size_t)kDdpFixedFloats + (size_t)net.num_params));
    }
  }
  if (hipError_t e = raise_lds_limit_once<ddp_fleet_kernel>(kDdpLdsLimit); e != hipSuccess) return e;
  hipLaunchKernelGGL(ddp_fleet_kernel, dim3(n), dim3(64 * kDdpFleetWaves), lds, stream, d_inst);
  return hipGetLastError();
}

hipError_t launch_device_tanhf(const float *in, float *out, size_t n, hipStream_t stream)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(device_tanhf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, out, n);
  return hipGetLastError();
}

}  // namespace mppi
