// ddp_fleet_device.hpp -- device functions of ddp_fleet.hip: ddp_feedback.cpp's pass for the network model on one workgroup,
// operation for operation.  Every sum is the host file's: k ascending from 0.0f with a SEPARATE multiply and add (the library is
// compiled -ffp-contract=off: write no fmaf here), the host's association, IEEE division, tanhf_scalar for tanhf.
// nominal_fleet.hip shares the forward layer (ddp_layer) with FMA = true: mppi_nominal_traj's arithmetic, where every multiply-add
// of a neuron's sum is one fmaf (host_net.hpp).  FMA = false is the DDP pass's text, unchanged.
#pragma once
#include "mppi_kernels.hpp"
#include "mppi_device.hpp"
#include "tanhf_scalar.hpp"

namespace mppi {

constexpr int kDdpAhead = 8;       // k steps of weights in flight (the forward layer)
constexpr int kDdpMaxWidth = 256;  // mppi_create's limit

// cwiseMin(u_max).cwiseMax(u_min): ddp_feedback.cpp's clamp_minmax, the same operand order
__device__ __forceinline__ float ddp_clamp_minmax(float v, float lo, float hi)
{
  v = (v < hi) ? v : hi;
  v = (v > lo) ? v : lo;
  return v;
}

// what one lane stored to the wave's tile is what every lane of the wave reads next
__device__ __forceinline__ void ddp_wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sinf / cosf of the heading: computed in double and rounded (glibc's sinf is not ported: DESIGN 4.20)
__device__ __forceinline__ void ddp_sincos(float psi, float &sn, float &cs)
{
  double s, c;
  sincos((double)psi, &s, &c);
  sn = (float)s;
  cs = (float)c;
}

// One layer of HostNet::forward for the wave: C chains per lane (neurons lane + 64 c), Wt the layer's k-major weights [nin][nout],
// b its biases: s = 0, k ascending s = s + W[j][k] * a[k], then s + b[j], then tanhf on a hidden layer.  th: where a hidden layer's
// tanh values are kept for the Jacobian (nullptr: not kept).  A lane past the layer's width walks the last neuron's weights and
// stores nothing.  The skeleton (weights requested kDdpAhead k steps ahead, activations as broadcast reads) is rollout_trace.hip's.
template <int C, bool FMA = false>
__device__ __forceinline__ void ddp_layer(const float *Wt, const float *b, int nin, int nout, bool hidden, const float *cur,
                                          float *nxt, float *th, int lane)
{
  int jj[C];
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; c++) {
    jj[c] = min(lane + 64 * c, nout - 1);
    acc[c] = 0.0f;
  }
  const int full = nin & ~(kDdpAhead - 1);
  float w[kDdpAhead][C];
  if (full > 0) {
#pragma unroll
    for (int u = 0; u < kDdpAhead; u++)
#pragma unroll
      for (int c = 0; c < C; c++) w[u][c] = Wt[u * nout + jj[c]];
  }
  for (int k0 = 0; k0 < full; k0 += kDdpAhead) {
    float wc[kDdpAhead][C];
#pragma unroll
    for (int u = 0; u < kDdpAhead; u++)
#pragma unroll
      for (int c = 0; c < C; c++) wc[u][c] = w[u][c];
    if (k0 + kDdpAhead < full) {  // the next chunk, requested before this one is multiplied
      const float *Wn = Wt + (size_t)(k0 + kDdpAhead) * nout;
#pragma unroll
      for (int u = 0; u < kDdpAhead; u++)
#pragma unroll
        for (int c = 0; c < C; c++) w[u][c] = Wn[u * nout + jj[c]];
    }
    float x[kDdpAhead];
#pragma unroll
    for (int q = 0; q < kDdpAhead / 4; q++) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(cur + k0 + 4 * q);  // broadcast: every lane the same address
      x[4 * q] = v[0]; x[4 * q + 1] = v[1]; x[4 * q + 2] = v[2]; x[4 * q + 3] = v[3];
    }
#pragma unroll
    for (int u = 0; u < kDdpAhead; u++)
#pragma unroll
      for (int c = 0; c < C; c++) {
        if constexpr (FMA) acc[c] = fmaf(wc[u][c], x[u], acc[c]);
        else acc[c] = acc[c] + wc[u][c] * x[u];
      }
  }
  for (int k = full; k < nin; k++) {  // the ragged end, one k at a time
    const float x = cur[k];
#pragma unroll
    for (int c = 0; c < C; c++) {
      if constexpr (FMA) acc[c] = fmaf(Wt[k * nout + jj[c]], x, acc[c]);
      else acc[c] = acc[c] + Wt[k * nout + jj[c]] * x;
    }
  }
#pragma unroll
  for (int c = 0; c < C; c++) {
    float y = acc[c] + b[jj[c]];
    if (hidden) y = tanhf_scalar(y);
    if (lane + 64 * c < nout) {
      nxt[lane + 64 * c] = y;
      if (hidden && th) th[lane + 64 * c] = y;
    }
  }
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
  ddp_wave_sync();
  float *cur = tile0, *nxt = tile1;
  int off = 0, hoff = 0;
  for (int l = 0; l + 1 < net.n_layers; l++) {
    const int nin = net.layers[l], nout = net.layers[l + 1];
    const float *Wt = img + off, *b = Wt + nin * nout;
    const bool hidden = l + 2 < net.n_layers;
    float *thl = (th && hidden) ? th + hoff : nullptr;
    const int chains = (nout + 63) >> 6;
    if (chains == 1) ddp_layer<1>(Wt, b, nin, nout, hidden, cur, nxt, thl, lane);
    else if (chains == 2) ddp_layer<2>(Wt, b, nin, nout, hidden, cur, nxt, thl, lane);
    else if (chains == 3) ddp_layer<3>(Wt, b, nin, nout, hidden, cur, nxt, thl, lane);
    else ddp_layer<4>(Wt, b, nin, nout, hidden, cur, nxt, thl, lane);
    ddp_wave_sync();
    off += nin * nout + nout;
    hoff += nout;
    float *sw = cur; cur = nxt; nxt = sw;
  }
  const f32x4 d = *reinterpret_cast<const f32x4 *>(cur);
  dx[3] = d[0]; dx[4] = d[1]; dx[5] = d[2]; dx[6] = d[3];
  ddp_wave_sync();  // the next step's inputs go to tile0, which may be the tile just read
}

// HostNet::jacobian_after_f of one step for the wave, scaled by dt and + I (ddp.h:71-80), and the step's cost derivatives:
// rec[0..63) = df (7 x 9, row-major), rec[63..72) = dL.  d0 / d1: the wave's two delta tiles, [kDdpMaxWidth] float4 (the four
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
  ddp_wave_sync();
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
    ddp_wave_sync();
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
  ddp_wave_sync();  // the tiles are the next step's
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
