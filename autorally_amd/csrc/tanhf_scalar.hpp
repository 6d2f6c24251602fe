// tanhf_scalar.hpp -- tanhf of one float, BIT FOR BIT the tanhf of the C library the reference's host code calls: the algorithm of
// tanhf_vec.hpp (glibc's s_tanhf.c on s_expm1f.c, every branch a select) as ONE scalar text for the host and the device.
//
// Why: the DDP kernel (ddp_fleet.hip) restates the host pass of ddp_feedback.cpp on the GPU, and the Riccati recursion turns a
// tanh difference of 1e-7 into 1e-3 of the feedforward term at T = 250 (tanhf_vec.hpp).  Every operation below is a
// plain IEEE single-precision operation -- multiply, add, subtract, divide, int <-> float conversion, integer work on the bit
// pattern -- which a gfx950 lane and an x86 core round alike; nothing here may be fused (compile with -ffp-contract=off, as the
// whole library is) and the division has to be the correctly rounded one (hipcc's default).  Compiled for the host by
// tests/test_ddp_fleet_cpu.py against libm; run on the device by mppi_debug_device_tanhf (tests/test_ddp_fleet_gpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MPPI_TANHF_HD __host__ __device__
#else
#define MPPI_TANHF_HD
#endif

namespace mppi {

MPPI_TANHF_HD static inline uint32_t tanhf_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
MPPI_TANHF_HD static inline float tanhf_float(uint32_t b) { return __builtin_bit_cast(float, b); }

MPPI_TANHF_HD static inline float tanhf_scalar(float x)
{
  const float one = 1.0f, two = 2.0f, half = 0.5f;
  const uint32_t jx = tanhf_bits(x);
  const uint32_t ix = jx & 0x7fffffffu;
  const float ax = tanhf_float(ix);  // fabsf(x)
  // tanhf: |x| >= 1 -> expm1f(2|x|), else expm1f(-2|x|)
  const bool ge1 = ix > 0x3f7fffffu;
  const float twoax = two * ax;
  const float a = ge1 ? twoax : -twoax;

  // ---- expm1f(a) ----
  const float ln2_hi = tanhf_float(0x3f317180u), ln2_lo = tanhf_float(0x3717f7d1u), invln2 = tanhf_float(0x3fb8aa3bu);
  const float Q1 = tanhf_float(0xbd088889u), Q2 = tanhf_float(0x3ad00d01u), Q3 = tanhf_float(0xb8a670cdu);
  const float Q4 = tanhf_float(0x36867e54u), Q5 = tanhf_float(0xb457edbbu);
  const uint32_t ab = tanhf_bits(a);
  const uint32_t hx = ab & 0x7fffffffu;
  const bool neg = (ab >> 31) != 0;
  // argument reduction
  const bool red = hx > 0x3eb17218u;   // |a| > 0.5 ln2
  const bool near = hx < 0x3F851592u;  // |a| < 1.5 ln2
  const float kf = invln2 * a + (neg ? -half : half);
  // truncated; tanhf reaches k in [-3, 63] wherever the result below is kept (|x| < 22): anything else (|x| >= 22, inf, NaN) is
  // replaced at the end, and takes k = 0 here so that no conversion or shift leaves its range
  int k = (kf > -64.0f && kf < 64.0f) ? (int)kf : 0;
  if (red && near && neg) k = -1;  // the special case |a| < 1.5 ln2 (a > 0 never comes here from tanhf: a >= 2)
  if (!red) k = 0;
  const float tk = (float)k;
  const float hi = a - tk * ln2_hi;  // t*ln2_hi is exact
  const float lo = tk * ln2_lo;
  const float xr = hi - lo;        // k = 0: hi = a, lo = 0 -> a
  const float c = (hi - xr) - lo;  // k = 0: 0
  // primary range
  const float hfx = half * xr;
  const float hxs = xr * hfx;
  float r1 = Q4 + hxs * Q5;
  r1 = Q3 + hxs * r1;
  r1 = Q2 + hxs * r1;
  r1 = Q1 + hxs * r1;
  r1 = one + hxs * r1;
  const float t3 = 3.0f - r1 * hfx;
  const float e = hxs * ((r1 - t3) / (6.0f - xr * t3));
  // k == 0: x - (x*e - hxs)
  const float r_k0 = xr - (xr * e - hxs);
  // k != 0
  float e2 = xr * (e - c) - c;
  e2 = e2 - hxs;
  const float r_km1 = half * (xr - e2) - half;  // 0.5*(x-e) - 0.5
  const uint32_t kshift = (uint32_t)k << 23;
  // k <= -2 || k > 56: y = one - (e - x); exponent += k; y - one
  const float y_a = tanhf_float(tanhf_bits(one - (e2 - xr)) + kshift);
  const float r_far = y_a - one;
  // 0 < k < 23: t = 1 - 2^-k; y = t - (e - x); exponent += k
  const int kpos = k > 0 ? k : 0;
  const float t_b = tanhf_float(0x3f800000u - (kpos < 32 ? (0x1000000u >> kpos) : 0u));
  const float y_b = tanhf_float(tanhf_bits(t_b - (e2 - xr)) + kshift);
  // 23 <= k <= 56: t = 2^-k; y = x - (e + t); y += one; exponent += k
  const float t_c = tanhf_float((uint32_t)(0x7f - k) << 23);
  const float y_c = tanhf_float(tanhf_bits((xr - (e2 + t_c)) + one) + kshift);
  float em1 = (k < 23) ? y_b : y_c;  // (k > 0 by exclusion)
  em1 = (k < -1 || k > 56) ? r_far : em1;
  em1 = (k == -1) ? r_km1 : em1;
  em1 = (k == 0) ? r_k0 : em1;
  em1 = (hx < 0x33000000u) ? a : em1;  // |a| < 2^-25: expm1f returns its argument

  // ---- tanhf ----
  const float den = em1 + two;
  const float z_ge1 = one - two / den;  // one - two/(t+two)
  const float z_lt1 = (-em1) / den;     // -t/(t+two)
  float z = ge1 ? z_ge1 : z_lt1;
  z = (ix > 0x41afffffu) ? one : z;  // |x| >= 22 (and +-inf): one - tiny == 1
  z = tanhf_float(tanhf_bits(z) ^ (jx & 0x80000000u));  // sign: (jx >= 0) ? z : -z
  z = (ix < 0x24000000u) ? x * (one + x) : z;  // |x| < 2^-55: x*(one+x); zero: x (the same expression gives +-0)
  z = (x != x) ? x + x : z;  // NaN
  return z;
}

}  // namespace mppi
