// nominal_fleet.hip -- the nominal trajectories of a whole fleet in ONE launch (mppi_nominal_traj_batch): grid (n), one workgroup
// per controller, its argument block read from an array in device memory (as ddp_fleet_kernel and rollout_fleet16_kernel read
// theirs).  The kernel restates mppi_nominal_traj for the network model statement for statement (abi_host.hip, host_net.hpp):
// record s, clamp u with the host's two branches, the kinematics as two fmaf, per neuron the k-ascending fmaf chain from 0 with
// the bias added afterwards, tanhf_scalar on hidden layers, s = fmaf(sd, dt, s).  Only sinf / cosf of the heading differ: they
// are the rounded double results (ddp_sincos), not glibc's floats.  The network is wave_net.hpp's per-wave forward with the host
// replay's neuron (WaveArithHostFma).
//
// The replay is one recurrence of T dependent steps: latency is the whole cost.  What is NOT on it:
//   * the heading of step t + 1 is fmaf(-+s6[t], dt, psi[t]), known before step t's network runs, so its sin / cos are computed
//     a step ahead;
//   * U[t + 1] is fetched a step ahead;
//   * control_seq does not depend on the state: the whole workgroup clamps and records it before the loop;
//   * the state records are stores nobody waits for.
// MPPI_NOMINAL_FLEET_WAVES = 2: wave 0 runs the network and the Euler step; inside the loop it only LOADS from global memory
// (U[t + 1]; the image's weights where the image is not in LDS), so no wait of its covers a store.  Wave 1, the rider, takes
// s[t] from an LDS slot, records it (stores only: it never waits for memory), computes sin / cos of psi[t + 1] in double and
// hands them over in an LDS slot -- one s_barrier per step, both slots double-buffered.  = 1: one wave does everything, the
// sin / cos issued ahead of the network (nom_single_wave, nominal_fleet_device.hpp: the text nominal_gains_fleet.hip runs beside the
// DDP pass's initial rollout).  DESIGN 4.21 has the measurement and which one is kept.
#include "../../include/mppi_hip.h"
#include "nominal_fleet_device.hpp"

namespace mppi {

#ifndef MPPI_NOMINAL_FLEET_WAVES
#define MPPI_NOMINAL_FLEET_WAVES 2  // waves per workgroup: 2 = network wave + rider, 1 = one wave (a build knob for A/B)
#endif
constexpr int kNomWaves = MPPI_NOMINAL_FLEET_WAVES;
static_assert(kNomWaves == 1 || kNomWaves == 2, "one wave, or the network wave and its rider");
constexpr int kNomActFloats = 2 * kWaveNetMaxWidth;  // the network wave's two activation tiles
constexpr int kNomX = kNomActFloats;             // [2][8]: s[t] on its way to the rider (slot t & 1; float 7 is padding)
constexpr int kNomSC = kNomX + 16;               // [2][4]: {sn, cs} of step t on its way to the network wave (slot t & 1; two floats of padding)
constexpr int kNomFixedFloats = kNomSC + 8;
constexpr size_t kNomLdsLimit = 96 * 1024;       // tiles + slots + image
static_assert((kNomFixedFloats & 3) == 0, "the image behind the slots is read in 16-byte pieces");


// the two waves meet: what either stored to LDS before is what the other reads after.  Only the LDS counter is waited for: the
// rider's record stores stay in flight.
__device__ __forceinline__ void nom_group_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The network wave of two (MPPI_NOMINAL_FLEET_WAVES = 2): T - 1 steps; of global memory it reads U[t + 1] a step ahead and the
// image's weights where the image is not in LDS, and stores nothing
__device__ __forceinline__ void nom_network_wave(const NominalFleetArgs &A, const float *img, float *lds, const float *in, int lane)
{
  const NetDesc &net = A.net;
  const int T = A.T, negate = A.negate_yaw_der;
  const float dt = A.dt;
  const float ulo0 = A.u_lo[0], ulo1 = A.u_lo[1], uhi0 = A.u_hi[0], uhi1 = A.u_hi[1];
  const float *U = in + 7;
  float *tile0 = lds, *tile1 = lds + kWaveNetMaxWidth, *hx = lds + kNomX;
  const float *hsc = lds + kNomSC;
  float s[7];
#pragma unroll
  for (int i = 0; i < 7; i++) s[i] = in[i];
  float n0 = U[0], n1 = U[1];
  for (int t = 0; t + 1 < T; t++) {
    const float u0 = nom_clamp(n0, ulo0, uhi0), u1 = nom_clamp(n1, ulo1, uhi1);
    n0 = U[2 * (t + 1)];  // the next step's, requested a step ahead (t + 1 < T)
    n1 = U[2 * (t + 1) + 1];
    const float sn = hsc[4 * (t & 1)], cs = hsc[4 * (t & 1) + 1];
    nom_step(net, img, tile0, tile1, negate, dt, s, u0, u1, sn, cs, lane);
    if (lane == 0) {
      float *slot = hx + 8 * ((t + 1) & 1);
      const f32x4 a = {s[0], s[1], s[2], s[3]}, b = {s[4], s[5], s[6], 0.0f};
      *reinterpret_cast<f32x4 *>(slot) = a;
      *reinterpret_cast<f32x4 *>(slot + 4) = b;
    }
    nom_group_sync();  // barrier t: s[t + 1] is the rider's, {sn, cs}[t + 1] this wave's
  }
}

// The rider: the state records, and step t + 1's sin / cos while step t's network runs.  It loads nothing from global memory, so
// none of its waits covers a record store.
__device__ __forceinline__ void nom_rider_wave(const NominalFleetArgs &A, float *lds, float *out, int lane)
{
  const int T = A.T, negate = A.negate_yaw_der;
  const float dt = A.dt;
  float *o_x = out;
  const float *hx = lds + kNomX;
  float *hsc = lds + kNomSC;
  for (int t = 0; t < T; t++) {
    const float *slot = hx + 8 * (t & 1);
    const float v = slot[lane & 7];
    if (lane < 7) o_x[(size_t)7 * t + lane] = v;
    if (t + 1 == T) break;
    const float psi = slot[2], s6 = slot[6];
    float sn, cs;
    ddp_sincos(fmaf(negate ? -s6 : s6, dt, psi), sn, cs);  // the network wave's Euler step of the heading, the same bits
    if (lane == 0) {
      hsc[4 * ((t + 1) & 1)] = sn;
      hsc[4 * ((t + 1) & 1) + 1] = cs;
    }
    nom_group_sync();  // barrier t
  }
}

__global__ __launch_bounds__(64 * kNomWaves) void nominal_fleet_kernel(const NominalFleetArgs *__restrict__ inst)
{
  extern __shared__ __attribute__((aligned(16))) float nom_lds[];
  const NominalFleetArgs &A = inst[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float *wimg = load_global_ptr(A.wimg);
  const float *in = load_global_ptr(A.in);
  float *out = load_global_ptr(A.out);
  const bool img_lds = A.img_lds != 0;
  if (img_lds) {
    const int np = A.net.num_params;
    wave_net_stage_image(nom_lds + kNomFixedFloats, wimg, np, 64 * kNomWaves);
  }
  {  // control_seq: every control clamped, by the whole workgroup
    const int T = A.T;
    const float ulo0 = A.u_lo[0], ulo1 = A.u_lo[1], uhi0 = A.u_hi[0], uhi1 = A.u_hi[1];
    nom_clamp_controls(in + 7, out + (size_t)7 * T, T, ulo0, ulo1, uhi0, uhi1, 64 * kNomWaves);
  }
  if constexpr (kNomWaves == 1) {
    __syncthreads();
    if (img_lds) nom_single_wave(A, A.dt, nom_lds + kNomFixedFloats, nom_lds, in, out, lane);
    else nom_single_wave(A, A.dt, wimg, nom_lds, in, out, lane);
  } else {
    if (wave == 1) {  // step 0's hand-overs, both directions
      float *hx = nom_lds + kNomX, *hsc = nom_lds + kNomSC;
      if (lane < 8) hx[lane] = in[min(lane, 6)];
      float sn, cs;
      ddp_sincos(in[2], sn, cs);
      if (lane == 0) {
        hsc[0] = sn;
        hsc[1] = cs;
      }
    }
    __syncthreads();
    // both waves pass T - 1 barriers, whatever the data
    if (wave == 1) nom_rider_wave(A, nom_lds, out, lane);
    else if (img_lds) nom_network_wave(A, nom_lds + kNomFixedFloats, nom_lds, in, lane);
    else nom_network_wave(A, wimg, nom_lds, in, lane);
  }
}

bool nominal_fleet_image_in_lds(const NetDesc &net)
{
  return wave_net_image_in_lds(net, kNomFixedFloats, kNomLdsLimit);
}

hipError_t launch_nominal_fleet(const NominalFleetArgs *h_inst, const NominalFleetArgs *d_inst, int n, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  if (n > kMaxFleet) return hipErrorInvalidValue;
  size_t lds = sizeof(float) * (size_t)kNomFixedFloats;
  for (int i = 0; i < n; i++) {
    const NetDesc &net = h_inst[i].net;
    if (!wave_net_valid(net) || h_inst[i].T < 2) return hipErrorInvalidValue;
    if (h_inst[i].img_lds) {
      if (!nominal_fleet_image_in_lds(net)) return hipErrorInvalidValue;
      lds = std::max(lds, sizeof(float) * ((size_t)kNomFixedFloats + (size_t)net.num_params));
    }
  }
  if (hipError_t e = raise_lds_limit_once<nominal_fleet_kernel>(kNomLdsLimit); e != hipSuccess) return e;
  hipLaunchKernelGGL(nominal_fleet_kernel, dim3(n), dim3(64 * kNomWaves), lds, stream, d_inst);
  return hipGetLastError();
}

}  // namespace mppi
