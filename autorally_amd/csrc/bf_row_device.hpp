// bf_row_device.hpp -- the dynamics step of the basis-function row form (rollout_bf_row.hip), shared with its microbenchmark
// (tools/ub/bf_row_ub.hip): a lane's part of the image, and d[j] of its rollout from s3..s6 and the step's controls.
#pragma once
#include "bf_device.hpp"
#include "group_roles.hpp"
#include "mppi_kernels.hpp"

namespace mppi {

// this lane's part of the image (pack_bf_row_weights): 16-B entry e of lane p = 4 j + y at float4 index e * 16 + p -- and what
// the step needs of it as REGISTERS: the marks as all-ones / all-zeros words, so that a select by a mark is one bit-select
// instruction on a register operand (32 of them per step and 8 v_cndmask, profiles/r16_b_bf_row_isa.txt)
struct BfRowLane {
  float w[kBfRowSlots], c[kBfRowSlots], rc[kBfRowSlots];
  unsigned marks;
  unsigned plain[kBfRowSlots];  // ~0: slot m is its numerator
  unsigned keep2, keep3;        // 0: slot 2 / 3 is zero unless u_x >= 0.1
  unsigned dbl, used6;          // ~0: slot 3 is the double quotient; slot 6 exists
  unsigned y0, y2, ylo, yodd;   // ~0: y == 0, y == 2, y < 2, y odd
  double kd, rcd;               // this lane's half of the two double quotients by u_x (below); RN(1 / c[3]) in double
};
__device__ __forceinline__ unsigned bf_ones(bool b)
{
  unsigned m = b ? 0xFFFFFFFFu : 0u;
  asm volatile("" : "+v"(m));  // a register from here on, not a condition to evaluate again
  return m;
}
__device__ __forceinline__ void bf_row_load(const float *pack, int p, BfRowLane &L)
{
  const float4 *pk = reinterpret_cast<const float4 *>(pack) + p;
  const float4 w0 = pk[0], w1 = pk[16], c0 = pk[32], c1 = pk[48], r0 = pk[64], r1 = pk[80];
  L.w[0] = w0.x; L.w[1] = w0.y; L.w[2] = w0.z; L.w[3] = w0.w; L.w[4] = w1.x; L.w[5] = w1.y; L.w[6] = w1.z;
  L.marks = __float_as_uint(w1.w);
  L.c[0] = c0.x; L.c[1] = c0.y; L.c[2] = c0.z; L.c[3] = c0.w; L.c[4] = c1.x; L.c[5] = c1.y; L.c[6] = c1.z;
  L.rc[0] = r0.x; L.rc[1] = r0.y; L.rc[2] = r0.z; L.rc[3] = r0.w; L.rc[4] = r1.x; L.rc[5] = r1.y; L.rc[6] = r1.z;
#pragma unroll
  for (int m = 0; m < kBfRowSlots; m++) L.plain[m] = bf_ones((L.marks & (kBfRowPlain << m)) != 0);
  // the switch reaches i = 9, 13, 14, 15 (car_bfs.cuh): slots 2 and 3
  L.keep2 = bf_ones((L.marks & (kBfRowBigOnly << 2)) == 0);
  L.keep3 = bf_ones((L.marks & (kBfRowBigOnly << 3)) == 0);
  L.dbl = bf_ones((L.marks & kBfRowDouble) != 0);
  L.used6 = bf_ones((L.marks & (kBfRowUsed << (kBfRowSlots - 1))) != 0);
  const int y = p & 3;
  L.y0 = bf_ones(y == 0); L.y2 = bf_ones(y == 2); L.ylo = bf_ones(y < 2); L.yodd = bf_ones((y & 1) != 0);
  L.kd = (y & 1) ? 0.35 : 0.45;
  L.rcd = 1.0 / (double)L.c[3];  // RN(1 / 40), RN(1 / 1600) of the double quotients (a correctly rounded division)
}

template <int Q>
__device__ __forceinline__ float bf_row_bc(float a)  // row_newbcast:Q (rollout_row.hip: row_bc)
{
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(a), 0x150 + Q, 0xF, 0xF, false));
}
__device__ __forceinline__ float bf_sel4(int y, float a0, float a1, float a2, float a3)
{
  const float lo = (y == 0) ? a0 : a1, hi = (y == 2) ? a2 : a3;
  return (y < 2) ? lo : hi;
}
// m ? a : b for a mark word m (v_bfi_b32)
__device__ __forceinline__ float bf_pick(unsigned m, float a, float b)
{
  const unsigned ua = __float_as_uint(a), ub = __float_as_uint(b);
  return __uint_as_float(ub ^ ((ua ^ ub) & m));  // one instruction in the ISA (profiles/r16_b_bf_row_isa.txt)
}
__device__ __forceinline__ float bf_pick4(const BfRowLane &L, float a0, float a1, float a2, float a3)
{
  return bf_pick(L.ylo, bf_pick(L.y0, a0, a1), bf_pick(L.y2, a2, a3));
}
__device__ __forceinline__ double bf_pick_d(unsigned m, double a, double b)
{
  const unsigned long long ua = __builtin_bit_cast(unsigned long long, a), ub = __builtin_bit_cast(unsigned long long, b);
  const unsigned al = (unsigned)ua, bl = (unsigned)ub, ah = (unsigned)(ua >> 32), bh = (unsigned)(ub >> 32);
  const unsigned lo = bl ^ ((al ^ bl) & m), hi = bh ^ ((ah ^ bh) & m);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double bf_swap1_d(double a)  // the value of lane ^ 1 (quad_perm [1,0,3,2])
{
  const unsigned long long ua = __builtin_bit_cast(unsigned long long, a);
  const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)ua, 0xB1, 0xF, 0xF, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(ua >> 32), 0xB1, 0xF, 0xF, false);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// The shared sub-expressions: the operations of basis_shared_common / basis_shared_fast (basis_funcs.hpp, bf_device.hpp) on
// the same operands, arranged for a wave whose 64 lanes would otherwise all walk the same two double divisions:
//   * .45 s6 / s4 and .35 s6 / s4 are ONE division instruction -- even y-threads take the first, odd ones the second (the
//     factor is the lane's L.kd) -- and a lane gets its neighbour's quotient by a quad_perm move (two words);
//   * the quotient (q - t) / (1 + q t) is computed whatever `big` says and selected afterwards: no exec-mask region in the step.
// Against the step with basis_shared_fast called as bf3 calls it (profiles/r16_b_bf_row_isa.txt, r16_c_bf_row_ub.txt): 31 instead
// of 43 double-precision instructions and no exec-mask region instead of two per step; the recurrence alone 895 instead of
// 1 014 cycles per step.
__device__ __forceinline__ void bf_row_shared(const BfRowLane &L, const float s4, const float s5, const float s6, const float u0,
                                              BasisShared &c)
{
  c.big = (s4 >= 0.100000001490116119384765625f);  // (double)s4 > .1  <=>  s4 >= 0.1f
  c.r54 = s5 / s4;
  const double d6 = (double)s6, d4 = (double)s4;
  const double mine = L.kd * d6 / d4, other = bf_swap1_d(mine);
  const double e45 = bf_pick_d(L.yodd, other, mine), e35 = bf_pick_d(L.yodd, mine, other);
  const float q = (float)((double)c.r54 + e45);
  c.B = (double)c.r54 - e35;
  float sn, cs;
  sincos_fast(u0, sn, cs);
  const float t = sn / cs;
  c.su = sn;
  float Aq = (q - t) / fmaf(q, t, 1.0f);
  asm volatile("" : "+v"(Aq));  // computed on every lane: no branch on `big`
  c.A = c.big ? Aq : -t;
}

// d[j] of this lane's rollout, in every lane of quad j: s3..s6 and the clamped controls of the step, this lane's y-thread
__device__ __forceinline__ float bf_row_deriv(const BfRowLane &L, const int y, const float s3, const float s4, const float s5,
                                              const float s6, const float u0, const float u1)
{
  BasisShared c;
  bf_row_shared(L, s4, s5, s6, u0, c);
  // the products of basis_funcs_from (basis_funcs.hpp), every lane all of them
  const float A = c.A, su = c.su, aA = fabsf(A);
  const float suA = su * A, suAa = suA * aA, A3 = (A * A) * A, suA3 = su * A3, AaA = A * aA;
  const float Bf = (float)c.B, Bf3 = (Bf * Bf) * Bf;
  const float s65 = s6 * s5, s64 = s6 * s4, s36 = s3 * s6, s34 = s3 * s4, s346 = s34 * s6, s44 = s4 * s4, s444 = s44 * s4;
  const float u11 = u1 * u1, u111 = u11 * u1;
  // this lane's numerators: basis function i = y + 4 m in slot m
  float n[kBfRowSlots];
  n[0] = bf_pick4(L, u1, s4, suA, suAa);
  n[1] = bf_pick4(L, suA3, s65, s6, s5);
  n[2] = bf_pick4(L, su, c.r54, A, AaA);
  n[3] = bf_pick4(L, A3, 0.0f, 0.0f, Bf3);
  n[4] = bf_pick4(L, s64, s3, s36, s34);
  n[5] = bf_pick4(L, s346, s44, s444, u11);
  n[6] = u111;
  float phi[kBfRowSlots];
#pragma unroll
  for (int m = 0; m < kBfRowSlots; m++) {
    const float q = div_const(n[m], L.c[m], L.rc[m]);
    // a plain basis function is the value itself, not value / 1: the quotient of +-inf by 1 is NaN in this form
    phi[m] = bf_pick(L.plain[m], n[m], q);
  }
  {  // phi[13] = B / 40 and phi[14] = B |B| / 1600: double quotients, rounded to float afterwards
    const double nd = (y == 1) ? c.B : c.B * fabs(c.B);
    const float qd = (float)div_const_d(nd, (double)L.c[3], L.rcd);
    phi[3] = bf_pick(L.dbl, qd, phi[3]);
  }
  {  // the switch: 0 unless u_x >= 0.1, where the slot's mark says so
    const unsigned bigm = c.big ? 0xFFFFFFFFu : 0u;
    phi[2] = __uint_as_float(__float_as_uint(phi[2]) & (bigm | L.keep2));
    phi[3] = __uint_as_float(__float_as_uint(phi[3]) & (bigm | L.keep3));
  }
  float part = 0.0f;
#pragma unroll
  for (int m = 0; m < kBfRowSlots - 1; m++) part = fmaf(L.w[m], phi[m], part);
  // slot 6 exists for y = 0 only (i = 24): the shorter chains end here (a seventh link 0 * phi would turn -0 into +0, inf into NaN)
  part = bf_pick(L.used6, fmaf(L.w[kBfRowSlots - 1], phi[kBfRowSlots - 1], part), part);
  // the partial sums in the order y = 0, 1, 2, 3, from +0 (basis_dynamics_dev)
  float acc = 0.0f + quad_bc<0>(part);
  acc = acc + quad_bc<1>(part);
  acc = acc + quad_bc<2>(part);
  acc = acc + quad_bc<3>(part);
  return acc;
}

}  // namespace mppi
