// nominal_fleet_device.hpp -- device functions of nominal_fleet.hip that nominal_gains_fleet.hip runs as well: mppi_nominal_traj's
// clamp, the network and the update of one step, and the replay on ONE wave (nom_single_wave).  nominal_fleet.hip has the plan and
// the two-wave form, which stays there: its barrier per step is the workgroup's.
#pragma once
#include "ddp_fleet_device.hpp"

namespace mppi {

// mppi_nominal_traj's clamp: the host's two branches, NaN passes through
__device__ __forceinline__ float nom_clamp(float u, float lo, float hi) { return u < lo ? lo : (u > hi ? hi : u); }

// control_seq: every control clamped, by the `threads` threads of the workgroup
__device__ __forceinline__ void nom_clamp_controls(const float *U, float *o_u, int T, float ulo0, float ulo1, float uhi0, float uhi1,
                                                   int threads)
{
  for (int i = threadIdx.x; i < 2 * T; i += threads) o_u[i] = (i & 1) ? nom_clamp(U[i], ulo1, uhi1) : nom_clamp(U[i], ulo0, uhi0);
}

// The network of one step for the wave (all 64 lanes hold the same s, u and results): HostNetFma::forward on [s3, s4, s5, s6, u0,
// u1].  Lane 0 writes the six inputs (no lane-indexed pick among registers: that would put the state into scratch memory).
__device__ __forceinline__ void nom_net(const NetDesc &net, const float *img, float *tile0, float *tile1, const float (&s)[7],
                                        float u0, float u1, float (&o)[4], int lane)
{
  if (lane == 0) {
    const f32x4 a = {s[3], s[4], s[5], s[6]};
    *reinterpret_cast<f32x4 *>(tile0) = a;
    tile0[4] = u0;
    tile0[5] = u1;
  }
  const f32x4 d = wave_net_forward<WaveArithHostFma>(net, img, tile0, tile1, nullptr, lane);
  o[0] = d[0]; o[1] = d[1]; o[2] = d[2]; o[3] = d[3];
}

// mppi_nominal_traj's update of one step: the kinematics, the network, the Euler step
__device__ __forceinline__ void nom_step(const NetDesc &net, const float *img, float *tile0, float *tile1, int negate, float dt,
                                         float (&s)[7], float u0, float u1, float sn, float cs, int lane)
{
  float sd[7];
  sd[0] = fmaf(cs, s[4], -(sn * s[5]));
  sd[1] = fmaf(sn, s[4], cs * s[5]);
  sd[2] = negate ? -s[6] : s[6];
  float o[4];
  nom_net(net, img, tile0, tile1, s, u0, u1, o, lane);
  sd[3] = o[0]; sd[4] = o[1]; sd[5] = o[2]; sd[6] = o[3];
#pragma unroll
  for (int i = 0; i < 7; i++) s[i] = fmaf(sd[i], dt, s[i]);
}

// One wave does everything.  A: the kernel's argument block (net, T, negate_yaw_der, the limits); dt: the replay's step; img: the
// image, in LDS or in global memory -- the caller has one call for each, so that the weights are read with LDS or global
// instructions, not flat ones; lds: the wave's two activation tiles; in: [7] state | [T][2] controls; o_x: [T][7] state_seq.
template <class Args>
__device__ __forceinline__ void nom_single_wave(const Args &A, float dt, const float *img, float *lds, const float *in, float *o_x, int lane)
{
  const NetDesc &net = A.net;
  const int T = A.T, negate = A.negate_yaw_der;
  const float ulo0 = A.u_lo[0], ulo1 = A.u_lo[1], uhi0 = A.u_hi[0], uhi1 = A.u_hi[1];
  const float *U = in + 7;
  float *tile0 = lds, *tile1 = lds + kWaveNetMaxWidth;
  float s[7];
#pragma unroll
  for (int i = 0; i < 7; i++) s[i] = in[i];
  float sn, cs;
  ddp_sincos(s[2], sn, cs);
  float n0 = U[0], n1 = U[1];
  for (int t = 0; t < T; t++) {
    const float u0 = nom_clamp(n0, ulo0, uhi0), u1 = nom_clamp(n1, ulo1, uhi1);
    if (t + 1 < T) {  // the next step's, requested a step ahead
      n0 = U[2 * (t + 1)];
      n1 = U[2 * (t + 1) + 1];
    }
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 7; q++) o_x[(size_t)7 * t + q] = s[q];
    }
    if (t + 1 == T) break;  // the host's last update is computed and dropped
    // the next heading is this one's Euler step, whose operands are all here: its sin / cos are issued ahead of the network
    float sn_n, cs_n;
    ddp_sincos(fmaf(negate ? -s[6] : s[6], dt, s[2]), sn_n, cs_n);
    nom_step(net, img, tile0, tile1, negate, dt, s, u0, u1, sn, cs, lane);
    sn = sn_n;
    cs = cs_n;
  }
}

}  // namespace mppi
