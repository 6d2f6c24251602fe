// ddp_fleet.hip -- DDP feedback gains for a whole fleet in ONE launch (mppi_compute_feedback_gains_batch): grid (n), one workgroup
// per controller, its argument block read from an array in device memory (the way rollout_fleet16_kernel reads its own).  The
// kernel restates ddp_feedback.cpp: ddp_feedback_gains for the network model operation for operation (ddp_fleet_device.hpp), so a
// handle's gains are those of its host pass up to sinf / cosf of the heading, which are the rounded double results here.
//
// A pass is three sequential recurrences of T steps and T independent Jacobians -- the latency shape:
//   A  initial rollout, wave 0: wave_net.hpp's per-wave forward (lane j owns neurons j, j + 64, j + 128, j + 192; activations through an
//      LDS tile as broadcast reads; weights from the k-major image, in LDS where it fits, else from global memory); x[t], the
//      clamped u[t], sin / cos of the heading and every hidden layer's tanh values are kept per step
//   B  the T - 1 Jacobians the backward pass reads, step t on wave t mod kDdpFleetWaves: lane = input neuron, four output chains per
//      lane, k ascending over the layer's outputs, the weights row-major (theta itself); scaled by dt, + I; the step's dL beside them
//   C  Riccati recursion, wave 0: an 8 x 8 padded tile is the wave's 64 lanes, lane (i, j) owns element (i, j) of every 7 x 7 /
//      2 x 7 product; column 7 of a tile carries the vector that goes with it (Vx beside Vxx, qx beside qxx, qu beside qux, lk
//      beside Lk), so that a vector's sum is its matrix's sum in the spare lanes
//   D  forward pass with the gains, wave 0: the wave of A; the per-step costs and their k-ascending total
// Any layer list mppi_create accepts (widths up to 256) is data.  A factorisation that is not `ok` ends the pass with status 1.
#include "../../include/mppi_hip.h"
#include "ddp_fleet_device.hpp"

namespace mppi {

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

__global__ __launch_bounds__(64 * kDdpFleetWaves) void ddp_fleet_kernel(const DdpFleetArgs *__restrict__ inst)
{
  extern __shared__ __attribute__((aligned(16))) float ddp_lds[];
  const DdpFleetArgs &A = inst[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float *theta = load_global_ptr(A.theta);
  const float *wimg = load_global_ptr(A.wimg);
  const float *in = load_global_ptr(A.in);
  float *out = load_global_ptr(A.out);
  float *work = load_global_ptr(A.work);
  const NetDesc &net = A.net;  // the layer list stays in the argument block: read where a layer begins
  const int H = A.T, negate = A.negate_yaw_der;
  const float dt = A.dt;
  const float ulo0 = A.u_lo[0], ulo1 = A.u_lo[1], uhi0 = A.u_hi[0], uhi1 = A.u_hi[1];
  const int hidden = ddp_fleet_hidden(net);

  const float *x0 = in, *tx = in + 7, *tu = in + 7 + (size_t)7 * H;
  float *o_fb = out, *o_ff = o_fb + (size_t)14 * H, *o_x = o_ff + (size_t)2 * H, *o_u = o_x + (size_t)7 * H, *o_cost = o_u + (size_t)2 * H;
  float *o_tail = o_cost + H;  // total_cost, status
  float *w_x = work, *w_u = w_x + (size_t)7 * H, *w_sc = w_u + (size_t)2 * H, *w_rec = w_sc + (size_t)2 * H, *w_th = w_rec + (size_t)72 * H;

  float *tile0 = ddp_lds, *tile1 = ddp_lds + kWaveNetMaxWidth;
  float *delta = ddp_lds + kDdpActFloats + wave * kDdpDeltaFloats;
  const float *img = wimg;
  if (A.img_lds) {
    float *img_s = ddp_lds + kDdpFixedFloats;
    wave_net_stage_image(img_s, wimg, net.num_params, 64 * kDdpFleetWaves);
    img = img_s;
  }
  __syncthreads();

  // ---- A: initial rollout (ddp.h:55-65) ----
  float xs[7];  // x[H - 1] afterwards (wave 0)
  if (wave == 0) {
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
  __syncthreads();  // wave 0's records (global memory) are the workgroup's

  // ---- B: Jacobians (scaled, + I) and cost derivatives of steps 0 .. H - 2 (ddp.h:71-80; the last step's are never read) ----
  for (int t = wave; t < H - 1; t += kDdpFleetWaves) {
    const float sn = w_sc[2 * t], cs = w_sc[2 * t + 1];
    ddp_jacobian(net, theta, w_th + (size_t)t * hidden, reinterpret_cast<f32x4 *>(delta),
                 reinterpret_cast<f32x4 *>(delta) + kWaveNetMaxWidth, w_x + (size_t)7 * t, w_u + 2 * t, tx + (size_t)7 * t, tu + 2 * t, sn,
                 cs, dt, A.Q, A.R, w_rec + (size_t)72 * t, lane);
  }
  __syncthreads();
  if (wave != 0) return;  // C and D are one wave's; no workgroup barrier below

  // ---- C: backward pass (ddp.h:83-123) ----
  float *R_ = delta;  // wave 0's
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
    return;
  }
  __threadfence_block();  // the gains (global memory, written by lanes of row 0) are read by every lane below
  wave_tile_sync();

  // ---- D: forward pass with alpha = 1 (ddp.h:125-152) ----
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

__global__ __launch_bounds__(256) void device_tanhf_kernel(const float *__restrict__ in, float *__restrict__ out, size_t n)
{
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = tanhf_scalar(in[i]);
}

bool ddp_fleet_image_in_lds(const NetDesc &net)
{
  return wave_net_image_in_lds(net, kDdpFixedFloats, kDdpLdsLimit);
}

hipError_t launch_ddp_fleet(const DdpFleetArgs *h_inst, const DdpFleetArgs *d_inst, int n, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  if (n > kMaxFleet) return hipErrorInvalidValue;
  size_t lds = sizeof(float) * (size_t)kDdpFixedFloats;
  for (int i = 0; i < n; i++) {
    const NetDesc &net = h_inst[i].net;
    if (!wave_net_valid(net) || h_inst[i].T < 2) return hipErrorInvalidValue;
    if (h_inst[i].img_lds) {
      if (!ddp_fleet_image_in_lds(net)) return hipErrorInvalidValue;
      lds = std::max(lds, sizeof(float) * ((size_t)kDdpFixedFloats + (size_t)net.num_params));
    }
  }
  if (hipError_t e = raise_lds_limit_once<ddp_fleet_kernel>(kDdpLdsLimit); e != hipSuccess) return e;
  hipLaunchKernelGGL(ddp_fleet_kernel, dim3(n), dim3(64 * kDdpFleetWaves), lds, stream, d_inst);
  return hipGetLastError();
}

hipError_t launch_device_tanhf(const float *in, float *out, size_t n, hipStream_t stream)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(device_tanhf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, out, n);
  return hipGetLastError();
}

}  // namespace mppi
