// m44_core.hpp -- the arithmetic the forms on v_mfma_f32_4x4x1 with A-matrix broadcast share (rollout_m44.hip: weights in
// registers; rollout_lds44.hip, rollout_lds128.hip: weights in LDS, any layer list; their group is m44_group.hpp): the accumulator type, the 4 x 4 transpose inside a quad that turns a
// layer's D (VGPR r = rollout r, lane n = neuron n) into the next layer's A (lane-in-quad = rollout, VGPR = neuron-in-quad),
// and the packed tanh of a D.
#pragma once
#include "mppi_device.hpp"

namespace mppi {

typedef float m44_f4 __attribute__((ext_vector_type(4)));

template <int Q>
__device__ __forceinline__ float m44_qp(float v)
{
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), Q, 0xF, 0xF, false));
}
// 4 x 4 transpose inside every quad: in[r] lane 4 b + j  ->  out[s] lane 4 b + i = in[i] lane 4 b + s
__device__ __forceinline__ void m44_transpose(const float (&in)[4], float (&out)[4], bool hi, bool od)
{
  float t[4];
  {  // exchange the off-diagonal 2 x 2 blocks (registers r <-> r ^ 2, lanes ^ 2)
    const float x0 = m44_qp<0x4E>(hi ? in[0] : in[2]);  // quad_perm [2,3,0,1]
    const float x1 = m44_qp<0x4E>(hi ? in[1] : in[3]);
    t[0] = hi ? x0 : in[0];
    t[2] = hi ? in[2] : x0;
    t[1] = hi ? x1 : in[1];
    t[3] = hi ? in[3] : x1;
  }
  {  // inside each 2 x 2 block (registers r <-> r ^ 1, lanes ^ 1)
    const float y0 = m44_qp<0xB1>(od ? t[0] : t[1]);  // quad_perm [1,0,3,2]
    const float y1 = m44_qp<0xB1>(od ? t[2] : t[3]);
    out[0] = od ? y0 : t[0];
    out[1] = od ? t[1] : y0;
    out[2] = od ? y1 : t[2];
    out[3] = od ? t[3] : y1;
  }
}

__device__ __forceinline__ void m44_tanh(const m44_f4 &d, float bs, float (&act)[4])
{
  const f32x2 a01 = tanh_bias2(f32x2{d[0], d[1]}, f32x2{bs, bs});
  const f32x2 a23 = tanh_bias2(f32x2{d[2], d[3]}, f32x2{bs, bs});
  act[0] = a01.x; act[1] = a01.y; act[2] = a23.x; act[3] = a23.y;
}

}  // namespace mppi
