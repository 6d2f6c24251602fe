// ddp_fleet_device.hpp -- device functions of ddp_fleet.hip: ddp_feedback.cpp's pass for the network model on one workgroup,
// operation for operation.  Every sum is the host file's: k ascending from 0.0f with a SEPARATE multiply and add (the library is
// compiled -ffp-contract=off: write no fmaf here), the host's association, IEEE division, tanhf_scalar for tanhf.
// The network's forward pass is wave_net.hpp's per-wave forward with the DDP pass's neuron (WaveArithHostMulAdd);
// nominal_fleet.hip takes ddp_sincos from here and runs the same forward with the host replay's neuron (WaveArithHostFma).
#pragma once
#include "mppi_kernels.hpp"
#include "mppi_device.hpp"
#include "wave_net.hpp"

namespace mppi {

// cwiseMin(u_max).cwiseMax(u_min): ddp_feedback.cpp's clamp_minmax, the same operand order
__device__ __forceinline__ float ddp_clamp_minmax(float v, float lo, float hi)
{
  v = (v < hi) ? v : hi;
  v = (v > lo) ? v : lo;
  return v;
}

// sinf / cosf of the heading: computed in double and rounded (glibc's sinf is not ported: DESIGN 4.20)
__device__ __forceinline__ void ddp_sincos(float psi, float &sn, float &cs)
{
  double s, c;
  sincos((double)psi, &s, &c);
  sn = (float)s;
  cs = (float)c;
}

// HostNet::f for the wave (all 64 lanes hold the same x, u, dx): computeKinematics + the network.  tile0 / tile1: the wave's two
// activation tiles in LDS; img: the k-major image (LDS or global); th: the step's tanh values [sum of hidden widths] or nullptr.
__device__ __forceinline__ void ddp_f(const NetDesc &net, const float *img, float *tile0, float *tile1, int negate_yaw_der,
                                      const float (&x)[7], float u0, float u1, float sn, float cs, float (&dx)[7], float *th,
                                      int lane)
{
  dx[0] = cs * x[4] - sn * x[5];
  dx[1] = sn * x[4] + cs * x[5];
  dx[2] = negate_yaw_der ? -x[6] : x[6];
  {
    const float lo = (lane == 0) ? x[3] : (lane == 1) ? x[4] : x[5];
    const float hi = (lane == 3) ? x[6] : (lane == 4) ? u0 : u1;
    if (lane < kNetIn) tile0[lane] = (lane < 3) ? lo : hi;
  }
  const f32x4 d = wave_net_forward<WaveArithHostMulAdd>(net, img, tile0, tile1, th, lane);
  dx[3] = d[0]; dx[4] = d[1]; dx[5] = d[2]; dx[6] = d[3];
}

// HostNet::jacobian_after_f of one step for the wave, scaled by dt and + I (ddp.h:71-80), and the step's cost derivatives:
// rec[0..63) = df (7 x 9, row-major), rec[63..72) = dL.  d0 / d1: the wave's two delta tiles, [kWaveNetMaxWidth] float4 (the four
// outputs' chains of a neuron side by side); theta: the weights row-major (the reference's layout); th: the step's tanh values.
__device__ __forceinline__ void ddp_jacobian(const NetDesc &net, const float *theta, const float *th, f32x4 *d0, f32x4 *d1,
                                             const float *x, const float *u, const float *tx, const float *tu, float sn, float cs,
                                             float dt, const float *Q, const float *R, float *rec, int lane)
{
  // delta[c][k]: derivative of output c wrt neuron k of the current layer; starts as the 4 x 4 identity at the output
  if (lane < 4) {
    f32x4 e = {0.0f, 0.0f, 0.0f, 0.0f};
    e[lane] = 1.0f;
    d0[lane] = e;
  }
  wave_tile_sync();
  f32x4 *d = d0, *dn = d1;
  int off = net.num_params, hoff = 0;
  for (int l = 1; l + 2 < net.n_layers; l++) hoff += net.layers[l];  // hidden layers below the last one
  for (int l = net.n_layers - 2; l >= 0; l--) {
    const int nin = net.layers[l], nout = net.layers[l + 1];
    off -= nin * nout + nout;
    if (l > 0 && l < net.n_layers - 2) hoff -= net.layers[l];  // -> the tanh values of layer l's inputs: hidden layer l - 1
    const float *W = theta + off;
    for (int i0 = 0; i0 < nin; i0 += 64) {
      const int i = min(i0 + lane, nin - 1);
      float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
      for (int k = 0; k < nout; k++) {
        const float w = W[(size_t)k * nin + i];
        const f32x4 dk = d[k];  // broadcast
#pragma unroll
        for (int c = 0; c < 4; c++) s[c] = s[c] + w * dk[c];
      }
      if (l > 0) {  // 1 - tanh(z)^2 with the forward pass's tanh value
        const float tz = th[hoff + i];
        const float zp = 1.0f - tz * tz;
#pragma unroll
        for (int c = 0; c < 4; c++) s[c] = s[c] * zp;
      }
      if (i0 + lane < nin) {
        const f32x4 o = {s[0], s[1], s[2], s[3]};
        dn[i0 + lane] = o;
      }
    }
    wave_tile_sync();
    f32x4 *sw = d; d = dn; dn = sw;
  }
  if (lane < 63) {
    const int r = lane / 9, c = lane - 9 * r;
    float v = 0.0f;
    if (r == 0) v = (c == 2) ? -sn * x[4] - cs * x[5] : (c == 4) ? cs : (c == 5) ? -sn : 0.0f;
    if (r == 1) v = (c == 2) ? cs * x[4] - sn * x[5] : (c == 4) ? sn : (c == 5) ? cs : 0.0f;
    if (r == 2) v = (c == 6) ? -1.0f : 0.0f;  // regardless of negate_yaw_der (reference quirk)
    if (r >= 3 && c >= 3) v = 0.0f + reinterpret_cast<const float *>(d)[4 * (c - 3) + (r - 3)];
    v = v * dt;
    if (r == c) v += 1.0f;
    rec[lane] = v;
  }
  if (lane < 9) rec[63 + lane] = (lane < 7) ? Q[lane] * (x[lane] - tx[lane]) : R[lane - 7] * (u[lane - 7] - tu[lane - 7]);
  wave_tile_sync();  // the tiles are the next step's
}

// x = A^{-1} b for the symmetric 2 x 2 A: ddp_feedback.cpp's Ldlt2 (Eigen::LDLT semantics: largest |diagonal| first)
struct DdpLdlt2 {
  int p;
  float l, d0, d1;
  bool ok;
  __device__ __forceinline__ DdpLdlt2(float a00, float a01, float a10, float a11)
  {
    p = (fabsf(a11) > fabsf(a00)) ? 1 : 0;
    d0 = p ? a11 : a00;
    const float aqp = p ? a01 : a10, aqq = p ? a00 : a11;
    l = aqp / d0;
    d1 = aqq - l * aqp;
    ok = isfinite(d0) && isfinite(d1) && isfinite(l) && d0 != 0.0f;
  }
  __device__ __forceinline__ void solve(float b0, float b1, float &x0, float &x1) const
  {
    const float z0 = p ? b1 : b0;
    const float z1 = (p ? b0 : b1) - l * z0;
    const float w0 = z0 / d0;
    const float w1 = (d1 != 0.0f) ? z1 / d1 : 0.0f;
    const float v1 = w1;
    const float v0 = w0 - l * v1;
    x0 = p ? v1 : v0;
    x1 = p ? v0 : v1;
  }
};

}  // namespace mppi
