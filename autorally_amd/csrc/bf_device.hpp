// bf_device.hpp -- device code of the basis-function model shared by its rollout kernels (rollout_bf.hip) and the trace
// kernel (rollout_trace.hip): the shared sub-expressions, W phi and computeStateDeriv, one lane per rollout.
#pragma once
#include "basis_funcs.hpp"
#include "mppi_device.hpp"

namespace mppi {

constexpr int kBfLanes = 64;

// Device form of the shared sub-expressions.  tan(atan(q) - u0) is evaluated through
// tan(a - b) = (tan a - tan b) / (1 + tan a tan b) with tan(atan q) = q, and sin u0 / tan u0 come from
// one sincos_fast: no atanf, no tanf, no large-argument reduction on the recurrence.  The reference's
// own device code composes CUDA's sinf / atanf / tanf (2-4 ulp each); this form stays within the same
// few ulp of the exact value (tests/test_basis_funcs.py: <= 2e-5 of the derivative's scale against the
// literal restatement).
__device__ __forceinline__ void basis_shared_fast(const float *s, float u0, BasisShared &c)
{
  float q, sn, cs;
  basis_shared_common(s, c, q);
  sincos_fast(u0, sn, cs);
  const float t = sn / cs;
  c.su = sn;
  c.A = c.big ? (q - t) / fmaf(q, t, 1.0f) : -t;
}

// W phi on the device: the same four i-mod-4 chains per output as basis_dynamics (basis_funcs.hpp), two
// outputs per packed multiply-add.  Wr is W transposed, [25] columns of four outputs, held in registers
// for the whole rollout (100 VGPRs; one wavefront per SIMD has 512), loaded once through LDS.
struct BfWeights {
  f32x4 col[kNumBfs];
  __device__ __forceinline__ void load(const float *Wt_s)
  {
#pragma unroll
    for (int i = 0; i < kNumBfs; i++) col[i] = *reinterpret_cast<const f32x4 *>(Wt_s + 4 * i);
  }
};
__device__ __forceinline__ void basis_dynamics_dev(const BfWeights &Wr, const float *phi, float *d)
{
  f32x2 acc01[kBfYThreads], acc23[kBfYThreads];
#pragma unroll
  for (int y = 0; y < kBfYThreads; y++) acc01[y] = acc23[y] = f32x2{0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < kNumBfs; i++) {
    const f32x4 w = Wr.col[i];
    const f32x2 p = {phi[i], phi[i]};
    acc01[i % kBfYThreads] = __builtin_elementwise_fma(f32x2{w[0], w[1]}, p, acc01[i % kBfYThreads]);
    acc23[i % kBfYThreads] = __builtin_elementwise_fma(f32x2{w[2], w[3]}, p, acc23[i % kBfYThreads]);
  }
  f32x2 s01 = {0.0f, 0.0f}, s23 = {0.0f, 0.0f};
#pragma unroll
  for (int y = 0; y < kBfYThreads; y++) {
    s01 = s01 + acc01[y];
    s23 = s23 + acc23[y];
  }
  d[0] = s01.x; d[1] = s01.y; d[2] = s23.x; d[3] = s23.y;
}

// computeStateDeriv: kinematics with the yaw rate always negated (generalized_linear.cu:212-217)
__device__ __forceinline__ void bf_state_deriv(const BfWeights &W_s, const float *s, float u0, float u1, float cpsi,
                                               float spsi, float *sd)
{
  sd[0] = fmaf(cpsi, s[4], -(spsi * s[5]));
  sd[1] = fmaf(spsi, s[4], cpsi * s[5]);
  sd[2] = -s[6];
  float phi[kNumBfs];
  BasisShared c;
  basis_shared_fast(s, u0, c);
  basis_funcs_from(s, u1, c, phi);
  basis_dynamics_dev(W_s, phi, sd + 3);
}

}  // namespace mppi
