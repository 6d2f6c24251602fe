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

// ---- the four phases of a pass (ddp_fleet.hip has the plan), each ONE text: ddp_fleet_kernel calls them, and so does
// nominal_gains_fleet_kernel (nominal_gains_fleet.hip), whose targets are what its own replay wave and prologue left in device memory.
// Args: the kernel's argument block (net, Q, R, Qf); DdpFleetVals: what the kernel read from it once; DdpFleetPtrs: where a
// handle's inputs, results and records are.

#ifndef MPPI_DDP_FLEET_WAVES
#define MPPI_DDP_FLEET_WAVES 4  // waves per workgroup; only phase B (the Jacobians) uses more than one (a build knob for A/B)
#endif
constexpr int kDdpFleetWaves = MPPI_DDP_FLEET_WAVES;
constexpr int kDdpActFloats = 2 * kWaveNetMaxWidth;                   // wave 0's two activation tiles
constexpr int kDdpDeltaFloats = 2 * 4 * kWaveNetMaxWidth;             // a wave's two delta tiles (float4 per neuron)
constexpr int kDdpFixedFloats = kDdpActFloats + kDdpFleetWaves * kDdpDeltaFloats;
constexpr size_t kDdpLdsLimit = 96 * 1024;                        // tiles + image
// phase C and D reuse wave 0's delta tiles: eleven 8 x 8 tiles, the step's record, the forward pass's row
constexpr int kRicPhi = 0, kRicB = 64, kRicVxx = 128, kRicBtV = 192, kRicPtV = 256, kRicQux = 320, kRicQxx = 384, kRicLk = 448,
              kRicVn = 512, kRicQuu = 576, kRicDl = 592, kRicRow = 608, kRicEnd = 672;
static_assert(kRicEnd <= kDdpDeltaFloats, "phase C fits wave 0's delta tiles");

struct DdpFleetVals {
  int H, negate, hidden;
  float dt, ulo0, ulo1, uhi0, uhi1;
};
struct DdpFleetPtrs {
  const float *theta, *img;    // the weights row-major (B); the k-major image, LDS or global (A, D)
  const float *x0, *tx, *tu;   // [7] | [H][7] | [H][2]
  float *o_fb, *o_ff, *o_x, *o_u, *o_cost, *o_tail;  // DdpFleetArgs::out
  float *w_x, *w_u, *w_sc, *w_rec, *w_th;            // DdpFleetArgs::work
  float *tile0, *tile1;        // wave 0's activation tiles
};
// out / work of one handle (mppi_kernels.hpp: DdpFleetArgs)
__device__ __forceinline__ void ddp_fleet_lay_out(DdpFleetPtrs &P, float *out, float *work, int H)
{
  P.o_fb = out; P.o_ff = P.o_fb + (size_t)14 * H; P.o_x = P.o_ff + (size_t)2 * H; P.o_u = P.o_x + (size_t)7 * H; P.o_cost = P.o_u + (size_t)2 * H;
  P.o_tail = P.o_cost + H;  // total_cost, status
  P.w_x = work; P.w_u = P.w_x + (size_t)7 * H; P.w_sc = P.w_u + (size_t)2 * H; P.w_rec = P.w_sc + (size_t)2 * H; P.w_th = P.w_rec + (size_t)72 * H;
}

#define DDP_FLEET_LOCALS                                                                                                   \
  const NetDesc &net = A.net;                                                                                              \
  const int H = V.H, negate = V.negate, hidden = V.hidden;                                                                 \
  const float dt = V.dt, ulo0 = V.ulo0, ulo1 = V.ulo1, uhi0 = V.uhi0, uhi1 = V.uhi1;                                       \
  const float *theta = P.theta, *img = P.img, *x0 = P.x0, *tx = P.tx, *tu = P.tu;                                          \
  float *o_fb = P.o_fb, *o_ff = P.o_ff, *o_x = P.o_x, *o_u = P.o_u, *o_cost = P.o_cost, *o_tail = P.o_tail;                \
  float *w_x = P.w_x, *w_u = P.w_u, *w_sc = P.w_sc, *w_rec = P.w_rec, *w_th = P.w_th, *tile0 = P.tile0, *tile1 = P.tile1;  \
  (void)net; (void)H; (void)negate; (void)hidden; (void)dt; (void)ulo0; (void)ulo1; (void)uhi0; (void)uhi1; (void)theta;   \
  (void)img; (void)x0; (void)tx; (void)tu; (void)o_fb; (void)o_ff; (void)o_x; (void)o_u; (void)o_cost; (void)o_tail;       \
  (void)w_x; (void)w_u; (void)w_sc; (void)w_rec; (void)w_th; (void)tile0; (void)tile1

// ---- A: initial rollout (ddp.h:55-65), one wave; xs: x[H - 1] afterwards ----
template <class Args>
__device__ __forceinline__ void ddp_phase_a(const Args &A, const DdpFleetVals &V, const DdpFleetPtrs &P, float (&xs)[7], int lane)
{
  DDP_FLEET_LOCALS;
#pragma unroll
  for (int i = 0; i < 7; i++) xs[i] = x0[i];
  float n0 = tu[0], n1 = tu[1];
  for (int i = 1; i < H; i++) {
    const int t = i - 1;
    float u0 = n0, u1 = n1;
    if (i < H - 1) {
      u0 = ddp_clamp_minmax(u0, ulo0, uhi0);
      u1 = ddp_clamp_minmax(u1, ulo1, uhi1);
      n0 = tu[2 * i];  // the next step's, requested a step ahead
      n1 = tu[2 * i + 1];
    }
    float sn, cs;
    ddp_sincos(xs[2], sn, cs);
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 7; q++) w_x[(size_t)7 * t + q] = xs[q];
      w_u[2 * t] = u0;
      w_u[2 * t + 1] = u1;
      w_sc[2 * t] = sn;
      w_sc[2 * t + 1] = cs;
    }
    float dx[7];
    ddp_f(net, img, tile0, tile1, negate, xs, u0, u1, sn, cs, dx, w_th + (size_t)t * hidden, lane);
#pragma unroll
    for (int q = 0; q < 7; q++) xs[q] = xs[q] + dx[q] * dt;
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 7; q++) w_x[(size_t)7 * (H - 1) + q] = xs[q];
  }
}

// ---- B: Jacobians (scaled, + I) and cost derivatives of steps 0 .. H - 2 (ddp.h:71-80; the last step's are never read), step t on
// wave t mod kDdpFleetWaves; delta: this wave's two delta tiles ----
template <class Args>
__device__ __forceinline__ void ddp_phase_b(const Args &A, const DdpFleetVals &V, const DdpFleetPtrs &P, float *delta, int wave, int lane)
{
  DDP_FLEET_LOCALS;
  for (int t = wave; t < H - 1; t += kDdpFleetWaves) {
    const float sn = w_sc[2 * t], cs = w_sc[2 * t + 1];
    ddp_jacobian(net, theta, w_th + (size_t)t * hidden, reinterpret_cast<f32x4 *>(delta),
                 reinterpret_cast<f32x4 *>(delta) + kWaveNetMaxWidth, w_x + (size_t)7 * t, w_u + 2 * t, tx + (size_t)7 * t, tu + 2 * t, sn,
                 cs, dt, A.Q, A.R, w_rec + (size_t)72 * t, lane);
  }
}

// ---- C: backward pass (ddp.h:83-123), one wave (the one of A: xs); delta: its delta tiles, phase D's as well.  Returns the status:
// 1 has written the tail and ends the pass ----
template <class Args>
__device__ __forceinline__ int ddp_phase_c(const Args &A, const DdpFleetVals &V, const DdpFleetPtrs &P, float *delta, const float (&xs)[7],
                                           float &Vlast_out, int lane)
{
  DDP_FLEET_LOCALS;
  float *R_ = delta;
  const int ri = lane >> 3, rj = lane & 7;
  const bool valid = ri < 7 && rj < 7;
  for (int q = lane; q < kRicEnd; q += 64) R_[q] = 0.0f;
  wave_tile_sync();
  float Vlast = 0.0f;
  {
    // boundary condition (target of the terminal cost = target_x[H-1])
#pragma unroll
    for (int i = 0; i < 7; i++) {
      const float e = xs[i] - tx[(size_t)7 * (H - 1) + i];
      Vlast += e * (A.Qf[i] * e);
    }
    if (ri < 7 && rj == ri) R_[kRicVxx + 8 * ri + rj] = A.Qf[ri];
    if (ri < 7 && rj == 7) {
      float xl = xs[0];
#pragma unroll
      for (int q = 1; q < 7; q++) xl = (ri == q) ? xs[q] : xl;
      const float e = xl - tx[(size_t)7 * (H - 1) + ri];
      R_[kRicVxx + 8 * ri + 7] = A.Qf[ri] * e;  // Vx
    }
  }
  const float qdt = (ri < 7) ? A.Q[ri] * dt : 0.0f;           // lane (i, i): qxx's diagonal term
  const float rdt = A.R[rj & 1] * dt;                        // lane (2 + j, j): quu's
  // the step's record [72]: df -> Phi | B, dL; lane l holds floats l and 64 + l
  float rec0 = 0.0f, rec1 = 0.0f;
  if (H >= 2) {
    const float *rec = w_rec + (size_t)72 * (H - 2);
    rec0 = rec[lane];
    if (lane < 8) rec1 = rec[64 + lane];
  }
  auto put_record = [&](float r0, float r1) {
    if (lane < 63) {
      const int r = lane / 9, c = lane - 9 * r;
      if (c < 7) R_[kRicPhi + 8 * r + c] = r0;
      else R_[kRicB + 8 * r + (c - 7)] = r0;
    } else {
      R_[kRicDl] = r0;  // float 63: dL[0]
    }
    if (lane < 8) R_[kRicDl + 1 + lane] = r1;
  };
  put_record(rec0, rec1);
  wave_tile_sync();
  int status = 0;
  for (int k = H - 2; k >= 0; k--) {
    if (k > 0) {  // the next step's record, requested now
      const float *rec = w_rec + (size_t)72 * (k - 1);
      rec0 = rec[lane];
      if (lane < 8) rec1 = rec[64 + lane];
    }
    // S1: Phi^T Vxx (column 7: Phi^T Vx -> qx) and B^T Vxx (column 7: B^T Vx -> qu)
    {
      float s = 0.0f, sb = 0.0f;
#pragma unroll
      for (int m = 0; m < 7; m++) {
        const float v = R_[kRicVxx + 8 * m + rj];
        s = s + R_[kRicPhi + 8 * m + ri] * v;
        sb = sb + R_[kRicB + 8 * m + (ri & 1)] * v;
      }
      if (ri < 7) {
        if (rj < 7) R_[kRicPtV + 8 * ri + rj] = s;
        else R_[kRicQxx + 8 * ri + 7] = R_[kRicDl + ri] * dt + s;  // qx
      }
      if (ri < 2) {
        if (rj < 7) R_[kRicBtV + 8 * ri + rj] = sb;
        else R_[kRicQux + 8 * ri + 7] = R_[kRicDl + 7 + ri] * dt + sb;  // qu
      }
    }
    wave_tile_sync();
    // S2: qxx = (Phi^T Vxx) Phi, qux = (B^T Vxx) Phi (lanes of rows 0, 1), quu = (B^T Vxx) B (lanes of rows 2, 3, columns 0, 1)
    {
      const int br = ri & 1;
      const float *Bm = (ri < 2) ? R_ + kRicPhi : R_ + kRicB;
      const int bj = (ri < 2) ? rj : (rj & 1);
      float s = 0.0f, sb = 0.0f;
#pragma unroll
      for (int m = 0; m < 7; m++) {
        s = s + R_[kRicPtV + 8 * ri + m] * R_[kRicPhi + 8 * m + rj];
        sb = sb + R_[kRicBtV + 8 * br + m] * Bm[8 * m + bj];
      }
      if (valid) R_[kRicQxx + 8 * ri + rj] = (ri == rj) ? qdt + s : s;
      if (ri < 2 && rj < 7) R_[kRicQux + 8 * ri + rj] = sb;
      if ((ri == 2 || ri == 3) && rj < 2) R_[kRicQuu + 2 * br + rj] = (br == rj) ? rdt + sb : sb;
    }
    wave_tile_sync();
    // S3: the pivoted 2 x 2 LDL^T (every lane), Lk's columns and lk (column 7) in the lanes of row 0
    {
      const DdpLdlt2 ldlt(R_[kRicQuu], R_[kRicQuu + 1], R_[kRicQuu + 2], R_[kRicQuu + 3]);
      if (!ldlt.ok) {
        status = 1;
        break;
      }
      if (ri == 0) {
        float s0, s1;
        ldlt.solve(-R_[kRicQux + rj], -R_[kRicQux + 8 + rj], s0, s1);
        R_[kRicLk + rj] = s0;
        R_[kRicLk + 8 + rj] = s1;
        if (rj < 7) {
          o_fb[(size_t)14 * k + rj] = s0;
          o_fb[(size_t)14 * k + 7 + rj] = s1;
        } else {
          o_ff[2 * k] = s0;
          o_ff[2 * k + 1] = s1;
        }
      }
    }
    wave_tile_sync();
    // S4: Vn = qxx + qux^T Lk; column 7: Vx = qx + (qux^T lk), whose sum has no leading zero in the host file
    {
      const float p0 = R_[kRicQux + ri] * R_[kRicLk + rj];
      float s = (rj == 7) ? p0 : 0.0f + p0;
      s = s + R_[kRicQux + 8 + ri] * R_[kRicLk + 8 + rj];
      const float v = R_[kRicQxx + 8 * ri + rj] + s;
      if (ri < 7) {
        if (rj < 7) R_[kRicVn + 8 * ri + rj] = v;
        else R_[kRicVxx + 8 * ri + 7] = v;
      }
    }
    wave_tile_sync();
    // S5: Vxx = 0.5 (Vn + Vn^T); the next step's record
    if (valid) R_[kRicVxx + 8 * ri + rj] = 0.5f * (R_[kRicVn + 8 * ri + rj] + R_[kRicVn + 8 * rj + ri]);
    if (k > 0) put_record(rec0, rec1);
    wave_tile_sync();
  }
  if (status != 0) {
    if (lane == 0) {
      o_tail[0] = 0.0f;
      o_tail[1] = __int_as_float(1);
    }
    return 1;
  }
  Vlast_out = Vlast;
  return 0;
}

// ---- D: forward pass with alpha = 1 (ddp.h:125-152), the wave of C ----
template <class Args>
__device__ __forceinline__ void ddp_phase_d(const Args &A, const DdpFleetVals &V, const DdpFleetPtrs &P, float *delta, float Vlast, int lane)
{
  DDP_FLEET_LOCALS;
  float *R_ = delta;
  __threadfence_block();  // the gains (global memory, written by lanes of row 0) are read by every lane below
  wave_tile_sync();

  float *row = R_ + kRicRow;  // [x 7 | u 2 | feedback 14 | feedforward 2 | target_x 7 | target_u 2] of the step
  auto row_addr = [&](int k) -> const float * {
    const int l = lane;
    if (l < 7) return w_x + (size_t)7 * k + l;
    if (l < 9) return w_u + 2 * k + (l - 7);
    if (l < 23) return o_fb + (size_t)14 * k + (l - 9);
    if (l < 25) return o_ff + 2 * k + (l - 23);
    if (l < 32) return tx + (size_t)7 * k + (l - 25);
    return tu + 2 * k + (min(l, 33) - 32);
  };
  float ox[7];
#pragma unroll
  for (int i = 0; i < 7; i++) ox[i] = x0[i];
  float tot = 0.0f;
  float rv = (H >= 2) ? *row_addr(0) : 0.0f;
  for (int k = 0; k + 1 < H; k++) {
    if (lane < 34) row[lane] = rv;
    wave_tile_sync();
    if (k + 2 < H) rv = *row_addr(k + 1);  // the next step's row, requested now
    float r[36];
#pragma unroll
    for (int q = 0; q < 9; q++) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(row + 4 * q);
      r[4 * q] = v[0]; r[4 * q + 1] = v[1]; r[4 * q + 2] = v[2]; r[4 * q + 3] = v[3];
    }
    wave_tile_sync();  // the row is the next step's from here
    float dxs[7];
#pragma unroll
    for (int i = 0; i < 7; i++) dxs[i] = ox[i] - r[i];
    float un[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
      float s = 0.0f;
#pragma unroll
      for (int i = 0; i < 7; i++) s += r[9 + 7 * j + i] * dxs[i];
      un[j] = (r[7 + j] + 1.0f * r[23 + j]) + s;
    }
    un[0] = ddp_clamp_minmax(un[0], ulo0, uhi0);
    un[1] = ddp_clamp_minmax(un[1], ulo1, uhi1);
    float sc = 0.0f, cc = 0.0f;
#pragma unroll
    for (int i = 0; i < 7; i++) {
      const float e = ox[i] - r[25 + i];
      sc += e * (A.Q[i] * e);
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const float e = un[j] - r[32 + j];
      cc += e * (A.R[j] * e);
    }
    const float ck = (sc + cc) * dt;
    tot += ck;
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 7; q++) o_x[(size_t)7 * k + q] = ox[q];
      o_u[2 * k] = un[0];
      o_u[2 * k + 1] = un[1];
      o_cost[k] = ck;
    }
    float sn, cs, fx[7];
    ddp_sincos(ox[2], sn, cs);
    ddp_f(net, img, tile0, tile1, negate, ox, un[0], un[1], sn, cs, fx, nullptr, lane);
#pragma unroll
    for (int i = 0; i < 7; i++) ox[i] = ox[i] + fx[i] * dt;
  }
  tot += Vlast;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 7; q++) o_x[(size_t)7 * (H - 1) + q] = ox[q];
    o_u[2 * (H - 1)] = 0.0f;
    o_u[2 * (H - 1) + 1] = 0.0f;
    o_ff[2 * (H - 1)] = 0.0f;
    o_ff[2 * (H - 1) + 1] = 0.0f;
    o_cost[H - 1] = Vlast;
    o_tail[0] = tot;
    o_tail[1] = __int_as_float(0);
  }
  if (lane < 14) o_fb[(size_t)14 * (H - 1) + lane] = 0.0f;
}
#undef DDP_FLEET_LOCALS

}  // namespace mppi
