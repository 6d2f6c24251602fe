// plant_drive_fleet.hip -- a plant of its own for a fleet (mppi_plant_drive_batch, mppi_closed_loop_sim_batch): grid (n), one
// workgroup of ONE wave per controller, its argument block read from an array in device memory -- plant_fleet_kernel's skeleton.
// The plant is a network of its own (mppi_set_plant_model) stepped `substeps` times per control period and driven by the law of
// include/mppi_hip.h, which plant_drive_host (abi_host.hip) states for the host: per plant step q, lo = q / m, j = q % m,
//   j == 0: u_ff, x_des, K are row lo;  j > 0: (1 - a) v[lo] + a v[lo + 1] in double with a = (double)j / (double)m, x_des and K
//   rounded to float, u kept in double;
//   feedback: du[c] = fmaf(K[c][i], x[i] - x_des[i], du[c]) for i ascending, added to u unless a du is NaN;
//   applied = nom_clamp((float)u[c], u_lo[c], u_hi[c]);  one step of nom_step's text with dt_sub = dt / (float)m.
// Only sin / cos of the heading differ from the host's text (ddp_sincos, as in nominal_fleet_kernel).
//
// The kernel is one controller's latency: periods * substeps dependent network evaluations between two solves of the loop.  On the
// chain from one step's Euler update to the next step's network stand x - x_des, the 14 fmaf, the add and the clamp.  Everything
// else of step q + 1 depends on nothing step q computes and is requested and finished while step q's network runs: the rows lo / hi
// (2 x (14 + 7 + 2) floats), their interpolation in double, and sin / cos of the next heading, fmaf(-+s6, dt_sub, psi).  Every lane
// computes the law; nothing is picked by lane index, so the state and the rows stay in registers.  lo and j are counted, not
// divided.  The image is in LDS or in global memory, one instantiation of the loop each (no flat loads): plant_drive_image_in_lds
// says which -- DESIGN 4.29 has the measurement.  Every loop bound is periods * substeps or a layer width, checked by
// launch_plant_drive_fleet; the kernel has no wait and no spin.
#include "../../include/mppi_hip.h"
#include "nominal_fleet_device.hpp"

namespace mppi {

constexpr int kDriveFixedFloats = 2 * kWaveNetMaxWidth;  // the wave's two activation tiles; the image behind them
constexpr size_t kDriveLdsLimit = 96 * 1024;
static_assert((kDriveFixedFloats & 3) == 0, "the image behind the tiles is read in 16-byte pieces");

// what the law needs of plant step (lo, j): u in double, x_des and K in float
struct DriveRows {
  double u0, u1;
  float xd[7], K[14];
};

__device__ __forceinline__ void drive_rows(const PlantDriveArgs &A, const float *U, const float *X, const float *G, int lo, int j,
                                           bool fb, bool clamp_rows, DriveRows &r)
{
  const float ulo0 = A.u_lo[0], ulo1 = A.u_lo[1], uhi0 = A.u_hi[0], uhi1 = A.u_hi[1];
  float l0 = U[2 * lo], l1 = U[2 * lo + 1];
  if (clamp_rows) {
    l0 = nom_clamp(l0, ulo0, uhi0);
    l1 = nom_clamp(l1, ulo1, uhi1);
  }
  if (j == 0) {  // nothing is interpolated: row lo + 1 is not read
    r.u0 = (double)l0;
    r.u1 = (double)l1;
    if (fb) {
#pragma unroll
      for (int i = 0; i < 7; i++) r.xd[i] = X[7 * lo + i];
#pragma unroll
      for (int i = 0; i < 14; i++) r.K[i] = G[14 * lo + i];
    }
    return;
  }
  const double a = A.a[j], b = 1.0 - a;
  float h0 = U[2 * lo + 2], h1 = U[2 * lo + 3];
  if (clamp_rows) {
    h0 = nom_clamp(h0, ulo0, uhi0);
    h1 = nom_clamp(h1, ulo1, uhi1);
  }
  r.u0 = b * (double)l0 + a * (double)h0;
  r.u1 = b * (double)l1 + a * (double)h1;
  if (fb) {
#pragma unroll
    for (int i = 0; i < 7; i++) r.xd[i] = (float)(b * (double)X[7 * lo + i] + a * (double)X[7 * lo + 7 + i]);
#pragma unroll
    for (int i = 0; i < 14; i++) r.K[i] = (float)(b * (double)G[14 * lo + i] + a * (double)G[14 * lo + 14 + i]);
  }
}

// The drive of one controller on its wave.  img: the plant's image, in LDS or in global memory (the caller has one call for each);
// lds: the wave's two activation tiles.
__device__ __forceinline__ void drive_wave(const PlantDriveArgs &A, const float *img, float *lds, const float *U, float *o_u, float (&s)[7],
                                           int lane)
{
  const NetDesc &net = A.net;
  const float *X = load_global_ptr(A.xseq);
  const float *G = load_global_ptr(A.gains);
  const int m = A.substeps, steps = A.periods * m, negate = A.negate_yaw_der;
  const bool fb = A.feedback != 0, clamp_rows = A.clamp_rows != 0;
  const float dt = A.dt_sub;
  const float ulo0 = A.u_lo[0], ulo1 = A.u_lo[1], uhi0 = A.u_hi[0], uhi1 = A.u_hi[1];
  float *tile0 = lds, *tile1 = lds + kWaveNetMaxWidth;
  DriveRows r;
  drive_rows(A, U, X, G, 0, 0, fb, clamp_rows, r);
  float sn, cs;
  ddp_sincos(s[2], sn, cs);
  int lo = 0, j = 0;
  for (int q = 0; q < steps; q++) {
    double u0 = r.u0, u1 = r.u1;
    if (fb) {
      float du0 = 0.0f, du1 = 0.0f;
#pragma unroll
      for (int i = 0; i < 7; i++) {
        const float e = s[i] - r.xd[i];
        du0 = fmaf(r.K[i], e, du0);
        du1 = fmaf(r.K[7 + i], e, du1);
      }
      if (!(du0 != du0) && !(du1 != du1)) {  // a NaN correction: feed-forward alone
        u0 += (double)du0;
        u1 += (double)du1;
      }
    }
    const float a0 = nom_clamp((float)u0, ulo0, uhi0), a1 = nom_clamp((float)u1, ulo1, uhi1);
    if (o_u != nullptr && lane == 0) {
      o_u[2 * q] = a0;
      o_u[2 * q + 1] = a1;
    }
    float sn_n = 0.0f, cs_n = 0.0f;
    if (q + 1 < steps) {  // the next step's rows, their interpolation and the sin / cos of its heading, ahead of this step's network
      if (++j == m) {
        j = 0;
        lo++;
      }
      drive_rows(A, U, X, G, lo, j, fb, clamp_rows, r);
      ddp_sincos(fmaf(negate ? -s[6] : s[6], dt, s[2]), sn_n, cs_n);
    }
    nom_step(net, img, tile0, tile1, negate, dt, s, a0, a1, sn, cs, lane);
    sn = sn_n;
    cs = cs_n;
  }
}

__global__ __launch_bounds__(64) void plant_drive_fleet_kernel(const PlantDriveArgs *__restrict__ inst, RolloutArgs *__restrict__ ra,
                                                               const int tick)
{
  extern __shared__ __attribute__((aligned(16))) float drive_lds[];
  const PlantDriveArgs &A = inst[blockIdx.x];
  const int lane = threadIdx.x;
  const float *wimg = load_global_ptr(A.wimg);
  const float *U = (tick & 1) ? load_global_ptr(A.useq_odd) : load_global_ptr(A.useq_even);
  const float *scal = load_global_ptr(A.scal);
  const float *state_in = load_global_ptr(A.state_in);
  float *state_out = load_global_ptr(A.state_out);
  float *applied = load_global_ptr(A.applied);
  float *log_x = load_global_ptr(A.log_x);
  const bool img_lds = A.img_lds != 0;
  if (img_lds) {
    wave_net_stage_image(drive_lds + kDriveFixedFloats, wimg, A.net.num_params, 64);
    __syncthreads();
  }
  float s[7];
#pragma unroll
  for (int i = 0; i < 7; i++) s[i] = state_in[i];
  if (scal != nullptr && lane == 0) {  // what the host checks behind a run, and the caller's cost log
    load_global_ptr(A.log_c)[tick] = scal[2];
    load_global_ptr(A.log_e)[tick] = scal[1];
  }
  float *o_u = applied != nullptr ? applied + (size_t)2 * A.periods * A.substeps * tick : nullptr;
  if (img_lds) drive_wave(A, drive_lds + kDriveFixedFloats, drive_lds, U, o_u, s, lane);
  else drive_wave(A, wimg, drive_lds, U, o_u, s, lane);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 7; q++) state_out[q] = s[q];
    if (log_x != nullptr) {
      float *o_x = log_x + (size_t)7 * (tick + 1);
#pragma unroll
      for (int q = 0; q < 7; q++) o_x[q] = s[q];
    }
    if (ra != nullptr) {
      float *next = ra[blockIdx.x].state;
#pragma unroll
      for (int q = 0; q < 7; q++) next[q] = s[q];
    }
  }
}

// does the image fit beside the tiles?  (whether a fitting image IS copied is the host's rule: plant_drive_wants_lds, abi_host.hip)
bool plant_drive_image_in_lds(const NetDesc &net)
{
  return wave_net_image_in_lds(net, kDriveFixedFloats, kDriveLdsLimit);
}

hipError_t launch_plant_drive_fleet(const PlantDriveArgs *h_inst, const PlantDriveArgs *d_inst, RolloutArgs *d_ra, int n, int tick, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  if (n > kMaxFleet || tick < 0) return hipErrorInvalidValue;
  size_t lds = sizeof(float) * (size_t)kDriveFixedFloats;
  for (int i = 0; i < n; i++) {
    const PlantDriveArgs &a = h_inst[i];
    if (!wave_net_valid(a.net) || a.net.layers[0] != kNetIn || a.net.layers[a.net.n_layers - 1] != kNetOut) return hipErrorInvalidValue;
    if (a.periods < 1 || a.substeps < 1 || a.substeps > kPlantDriveMaxSubsteps) return hipErrorInvalidValue;
    if (a.feedback && (!a.xseq || !a.gains)) return hipErrorInvalidValue;
    if (!a.wimg || !a.useq_even || !a.useq_odd || !a.state_in || !a.state_out) return hipErrorInvalidValue;
    if (a.scal && (!a.log_c || !a.log_e)) return hipErrorInvalidValue;
    if (a.img_lds) {
      if (!plant_drive_image_in_lds(a.net)) return hipErrorInvalidValue;
      lds = std::max(lds, sizeof(float) * ((size_t)kDriveFixedFloats + (size_t)a.net.num_params));
    }
  }
  if (hipError_t e = raise_lds_limit_once<plant_drive_fleet_kernel>(kDriveLdsLimit); e != hipSuccess) return e;
  hipLaunchKernelGGL(plant_drive_fleet_kernel, dim3(n), dim3(64), lds, stream, d_inst, d_ra, tick);
  return hipGetLastError();
}

}  // namespace mppi
