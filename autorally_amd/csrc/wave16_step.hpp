// wave16_step.hpp -- the WAVE of the forms that do the whole step on v_mfma_f32_16x16x4_f32 (rollout_mfma_kernel in
// rollout_mfma.hip, rollout_lds16.hip, rollout_glb16.hip): one wavefront = 16 rollouts, lane l = (rollout j = l & 15, k-slot /
// row group g = l >> 4), eps from the stand-alone generator, no rings, no riders, no barrier in the T loop.  Here, once:
// everything of rolloutKernel (PI/mppi_controller.cu:72-184) that is not the network.  A form adds its network as a policy
// object that its kernel constructs (the staging of an image and its barrier stay in the kernel, in front of the call):
//   typename Net::Step      what the network keeps from one piece of a step to the next (declared per step: no value of it
//                           outlives the step)
//   net.load(lane)          once, behind the exit of the absent waves: the lane's weights or its pointers into the image
//   net.request(x)          top of a step: what the network wants requested in front of the control arithmetic
//   net.layer0(x, g, s3, s4, s5, s6, u0, u1)   region 1: layer 0 from k-steps [s3, s4, s5, s6][g] and [u0, u1, 0, 0][g]
//   net.hidden(x, g)        region 2: the hidden layers
//   net.output(x, d)        region 3: the output layer into d[4], the bias added after the chain
// Every member is __forceinline__: a kernel's instruction stream is that of the step written out in it
// (profiles/r20_a_wave16_isa.txt).
#pragma once
#include "mppi_device.hpp"

namespace mppi {

// a by value, not by reference: inlined, the copy is the kernel's argument block again.  Through a reference the 6-64x4-4
// instance of rollout_mfma_kernel, which has no register to spare, came out with a tenth fewer packed instructions and 2.7 %
// slower; by value its registers and its packed arithmetic are the parent's (profiles/r20_a_wave16_isa.txt, r20_c_wave16_times.txt)
template <bool AFFINE, bool CTRL, class Net>
__device__ __forceinline__ void wave16_rollout(const RolloutArgs a, Net &net)
{
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (wave * kRolloutsPerWave >= a.K) return;  // whole wave (K is a multiple of 64)
  const int j = lane & 15, g = lane >> 4;
  const int k = wave * kRolloutsPerWave + j;
  net.load(lane);

  float s[kStateDim];
#pragma unroll
  for (int i = 0; i < kStateDim; i++) s[i] = a.state[i];
  int crash = 0;
  float J = 0.0f;

  const int K = a.K, T = a.T;
  float2 *const noise = reinterpret_cast<float2 *>(a.noise);
  const float2 *const Useq = reinterpret_cast<const float2 *>(a.U);
  const bool noise_free_k = (k == 0);       // mppi_controller.cu:136
  const bool pure_noise_k = (k >= a.k99);   // :141, k >= .99*NUM_ROLLOUTS in double (host)

  // Everything a step reads from memory is requested ahead of its use (noise line, nominal
  // control and 1/t one step ahead; the two costmap texels two network layers ahead), so no
  // load latency sits on the T-step recurrence.  A step is branch-free and cut into four
  // scheduling regions: in each, the MFMAs of one network piece run next to independent
  // cost / kinematics arithmetic.
  float2 eps = noise[(size_t)k];            // t = 0
  float2 Unext = Useq[0];
  double rt_next = a.inv_t[0];
  for (int t = 0; t < T; t++) {
    // ---- region 1: controls, layer 0, sin/cos, costmap addresses and fetches ----
    typename Net::Step x;
    net.request(x);
    const float2 e = eps;
    const float2 Ut = Unext;
    const double rt = rt_next;
    const int tn = min(t + 1, T - 1);
    eps = noise[(size_t)tn * K + k];
    Unext = Useq[tn];
    rt_next = a.inv_t[tn];
    // control perturbation, mppi_controller.cu:136-153
    const bool nf = noise_free_k | (t < a.opt_delay);
    const float n0 = e.x * a.nu[0], n1 = e.y * a.nu[1];
    const float du0 = nf ? 0.0f : n0, du1 = nf ? 0.0f : n1;
    float u0 = nf ? Ut.x : (pure_noise_k ? n0 : Ut.x + n0);
    float u1 = nf ? Ut.y : (pure_noise_k ? n1 : Ut.y + n1);
    // stored before the clamp (Q3); the four lanes of a rollout write the same value
    noise[(size_t)t * K + k] = make_float2(u0, u1);
    u0 = clampf(u0, a.u_lo[0], a.u_hi[0]);
    u1 = clampf(u1, a.u_lo[1], a.u_hi[1]);
    net.layer0(x, g, s[3], s[4], s[5], s[6], u0, u1);
    float spsi, cpsi;
    sincos_fast(s[2], spsi, cpsi);
    float tf, tb;
    track_fetch<AFFINE>(a.cost, s, cpsi, spsi, tf, tb);
    __builtin_amdgcn_sched_barrier(0);

    // ---- region 2: hidden layers next to kinematics and the texel-free cost terms ----
    net.hidden(x, g);
    float sd[kStateDim];
    sd[0] = fmaf(cpsi, s[4], -(spsi * s[5]));  // computeKinematics, neural_net_model.cu:346-355
    sd[1] = fmaf(spsi, s[4], cpsi * s[5]);
    sd[2] = a.negate_yaw_der ? -s[6] : s[6];
    CostTerms ct;
    cost_terms_a<CTRL>(a.cost, a.nu, s[4], s[5], u0, u1, du0, du1, ct);
    __builtin_amdgcn_sched_barrier(0);

    // ---- region 3: output layer next to the track / crash terms and the running mean ----
    float d[4];
    net.output(x, d);
    {
      // running mean over t = 1..T-1 of the cost of the state before the update (Q5); the
      // t = 0 evaluation is computed and discarded
      int crash_new = crash;
      const float c = cost_terms_b(a.cost, ct, tf, tb, crash_new);
      const float Jn = running_mean(J, c, t, rt);
      J = (t > 0) ? Jn : J;
      crash = (t > 0) ? crash_new : crash;
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- region 4: incrementState (:334-344) and getCrash (costs.cu:301-305) ----
    sd[3] = d[0]; sd[4] = d[1]; sd[5] = d[2]; sd[6] = d[3];
#pragma unroll
    for (int i = 0; i < kStateDim; i++) s[i] = fmaf(sd[i], a.dt, s[i]);
    crash |= (int)(fabsf(s[3]) >= kRollCrash);
  }
  if (g == 0) a.costs[k] = J + 0.0f;  // + terminalCost (= 0), costs.cu:411-414
}

}  // namespace mppi
