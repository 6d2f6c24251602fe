// plant_fleet.hip -- the plant step of a fleet's closed loop (mppi_closed_loop_ticks_batch): grid (n), one workgroup of ONE wave
// per controller, its argument block read from an array in device memory (as nominal_fleet_kernel reads its own).  The plant is
// the controller's own dynamics model: `stride` steps of mppi_nominal_traj's replay with the sequence the tail kernel has just
// smoothed -- nominal_fleet_device.hpp's text (nom_clamp, nom_step, the network as wave_net.hpp's forward with the host replay's
// neuron, ddp_sincos of the heading), so the new state is bit for bit row `stride` of nominal_fleet_kernel's state_seq and the
// logged controls are its first `stride` control_seq rows.
//
// The kernel runs between two solves on the fleet's stream: behind the argument copy of the NEXT tick, whose RolloutArgs::state it
// overwrites in device memory (plain vector stores from lane 0; the rollout launch behind it reads the block as every fleet launch
// does), and in front of that tick's generator and rollout.  Its length is on the loop's critical path, and it is latency: one
// image read per step, a layer's weights requested kWaveNetAhead k steps ahead.  The image stays in global memory: with the usual
// stride of 1 every weight is read exactly once, and a copy to LDS would be a second pass over it.
#include "../../include/mppi_hip.h"
#include "nominal_fleet_device.hpp"

namespace mppi {

__global__ __launch_bounds__(64) void plant_fleet_kernel(const PlantFleetArgs *__restrict__ inst, RolloutArgs *__restrict__ ra, const int tick)
{
  __shared__ __attribute__((aligned(16))) float plant_lds[2 * kWaveNetMaxWidth];  // the wave's two activation tiles
  const PlantFleetArgs &A = inst[blockIdx.x];
  const int lane = threadIdx.x;
  const float *wimg = load_global_ptr(A.wimg);
  const float *U = (tick & 1) ? load_global_ptr(A.U_odd) : load_global_ptr(A.U_even);
  const float *scal = load_global_ptr(A.scal);
  float *state = load_global_ptr(A.state);
  float *log_x = load_global_ptr(A.log_x);
  float *log_u = load_global_ptr(A.log_u);
  float *log_c = load_global_ptr(A.log_c);
  float *log_e = load_global_ptr(A.log_e);
  const NetDesc &net = A.net;
  const int stride = A.stride, negate = A.negate_yaw_der;
  const float dt = A.dt;
  const float ulo0 = A.u_lo[0], ulo1 = A.u_lo[1], uhi0 = A.u_hi[0], uhi1 = A.u_hi[1];
  float *tile0 = plant_lds, *tile1 = plant_lds + kWaveNetMaxWidth;
  float s[7];
#pragma unroll
  for (int i = 0; i < 7; i++) s[i] = state[i];
  float n0 = U[0], n1 = U[1];
  if (lane == 0) {  // what the host checks behind the run, and the caller's cost log
    log_c[tick] = scal[2];
    log_e[tick] = scal[1];
  }
  float sn, cs;
  ddp_sincos(s[2], sn, cs);
  float *o_u = log_u + (size_t)2 * stride * tick;
  for (int t = 0; t < stride; t++) {
    const float u0 = nom_clamp(n0, ulo0, uhi0), u1 = nom_clamp(n1, ulo1, uhi1);
    float sn_n = 0.0f, cs_n = 0.0f;
    if (t + 1 < stride) {  // the next step's controls and the sin / cos of its heading, requested ahead of this step's network
      n0 = U[2 * (t + 1)];
      n1 = U[2 * (t + 1) + 1];
      ddp_sincos(fmaf(negate ? -s[6] : s[6], dt, s[2]), sn_n, cs_n);
    }
    if (lane == 0) {
      o_u[2 * t] = u0;
      o_u[2 * t + 1] = u1;
    }
    nom_step(net, wimg, tile0, tile1, negate, dt, s, u0, u1, sn, cs, lane);
    sn = sn_n;
    cs = cs_n;
  }
  if (lane == 0) {
    float *o_x = log_x + (size_t)7 * (tick + 1);
#pragma unroll
    for (int q = 0; q < 7; q++) {
      state[q] = s[q];
      o_x[q] = s[q];
    }
    if (ra != nullptr) {
      float *next = ra[blockIdx.x].state;
#pragma unroll
      for (int q = 0; q < 7; q++) next[q] = s[q];
    }
  }
}

hipError_t launch_plant_fleet(const PlantFleetArgs *h_inst, const PlantFleetArgs *d_inst, RolloutArgs *d_ra, int n, int tick, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  if (n > kMaxFleet || tick < 0) return hipErrorInvalidValue;
  for (int i = 0; i < n; i++)
    if (!wave_net_valid(h_inst[i].net) || h_inst[i].T < 2 || h_inst[i].stride < 1 || h_inst[i].stride >= h_inst[i].T) return hipErrorInvalidValue;
  hipLaunchKernelGGL(plant_fleet_kernel, dim3(n), dim3(64), 0, stream, d_inst, d_ra, tick);
  return hipGetLastError();
}

}  // namespace mppi
