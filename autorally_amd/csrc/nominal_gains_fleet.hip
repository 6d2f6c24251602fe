// nominal_gains_fleet.hip -- the two closing stages of a fleet's tick in ONE launch (mppi_nominal_and_gains_batch): per controller the
// nominal replay of nominal_fleet.hip and the DDP pass of ddp_fleet.hip that tracks it.  Grid (n), one workgroup of four waves per
// controller, its argument block read from an array in device memory (as ddp_fleet_kernel reads its own).
//
// The pass's phase A (the initial rollout) never reads the target states, only the target controls -- which are the clamped
// control sequence, known before anything runs.  So:
//   before the loop  the whole workgroup clamps the control sequence with the replay's two branches and stores control_seq: the
//                    target controls tu of everything below
//   wave 0           phase A on tu (ddp_phase_a, the text ddp_fleet_kernel runs)
//   wave 1           the nominal replay at the same time, the one-wave form (nom_single_wave, the text nominal_fleet.hip keeps for
//                    MPPI_NOMINAL_FLEET_WAVES = 1): it writes state_seq, the target states tx.  The two-wave replay does not fit:
//                    its barrier per step is the workgroup's, and wave 0 passes none.
//   waves 2, 3       wait
// The waves meet once, at the barrier that ends phase A in ddp_fleet_kernel as well; there is no other hand-over between waves 0
// and 1.  Phases B, C and D follow as in ddp_fleet_kernel and read tx / tu from device memory.  Per controller the results are
// bit for bit those of nominal_fleet_kernel followed by ddp_fleet_kernel on its outputs: clamping a clamped control again returns
// it, and the one-wave and the two-wave replay run the same statements.
//
// LDS: ddp_fleet_kernel's tiles (wave 0's two activation tiles, every wave's two delta tiles), then the replay wave's two
// activation tiles of its own, then the weight image where all of it fits 96 KiB -- else both waves read the image from global
// memory.  The body is instantiated per image source, so that the weights are read with LDS or global instructions, not flat ones.
#include "../../include/mppi_hip.h"
#include "nominal_fleet_device.hpp"

namespace mppi {

constexpr int kNgReplayTiles = kDdpFixedFloats;                         // the replay wave's two activation tiles
constexpr int kNgFixedFloats = kNgReplayTiles + 2 * kWaveNetMaxWidth;
constexpr size_t kNgLdsLimit = 96 * 1024;                               // tiles + image
static_assert(kDdpFleetWaves >= 2, "wave 0 runs phase A, wave 1 the replay");
static_assert((kNgFixedFloats & 3) == 0, "the image behind the tiles is read in 16-byte pieces");

template <bool kImgLds>
__device__ __forceinline__ void nominal_gains_body(const NominalGainsFleetArgs &A, float *lds, int lane, int wave)
{
  const float *wimg = load_global_ptr(A.wimg);
  const float *in = load_global_ptr(A.in);
  float *out = load_global_ptr(A.out);
  DdpFleetPtrs P;
  P.theta = load_global_ptr(A.theta);
  DdpFleetVals V;
  V.H = A.T; V.negate = A.negate_yaw_der;
  V.dt = A.dt;
  V.ulo0 = A.u_lo[0]; V.ulo1 = A.u_lo[1]; V.uhi0 = A.u_hi[0]; V.uhi1 = A.u_hi[1];
  V.hidden = ddp_fleet_hidden(A.net);
  float *state_seq = out + (((size_t)26 * V.H + 2 + 3) & ~(size_t)3);  // nominal_gains_fleet_seq_offset
  float *control_seq = state_seq + (size_t)7 * V.H;
  P.x0 = in; P.tx = state_seq; P.tu = control_seq;
  ddp_fleet_lay_out(P, out, load_global_ptr(A.work), V.H);
  P.tile0 = lds; P.tile1 = lds + kWaveNetMaxWidth;
  float *delta = lds + kDdpActFloats + wave * kDdpDeltaFloats;
  if constexpr (kImgLds) {
    wave_net_stage_image(lds + kNgFixedFloats, wimg, A.net.num_params, 64 * kDdpFleetWaves);
    P.img = lds + kNgFixedFloats;
  } else {
    P.img = wimg;
  }
  nom_clamp_controls(in + 7, control_seq, V.H, V.ulo0, V.ulo1, V.uhi0, V.uhi1, 64 * kDdpFleetWaves);
  __syncthreads();  // the image (LDS) and tu (global memory) are the workgroup's

  float xs[7];  // x[H - 1] afterwards (wave 0)
  if (wave == 0) ddp_phase_a(A, V, P, xs, lane);
  else if (wave == 1) nom_single_wave(A, A.dt_nominal, P.img, lds + kNgReplayTiles, in, state_seq, lane);
  __syncthreads();  // wave 0's records and wave 1's tx (global memory) are the workgroup's
  ddp_phase_b(A, V, P, delta, wave, lane);
  __syncthreads();
  if (wave != 0) return;  // C and D are one wave's; no workgroup barrier below
  float Vlast;
  if (ddp_phase_c(A, V, P, delta, xs, Vlast, lane) != 0) return;
  ddp_phase_d(A, V, P, delta, Vlast, lane);
}

__global__ __launch_bounds__(64 * kDdpFleetWaves) void nominal_gains_fleet_kernel(const NominalGainsFleetArgs *__restrict__ inst)
{
  extern __shared__ __attribute__((aligned(16))) float ng_lds[];
  const NominalGainsFleetArgs &A = inst[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (A.img_lds) nominal_gains_body<true>(A, ng_lds, lane, wave);
  else nominal_gains_body<false>(A, ng_lds, lane, wave);
}

bool nominal_gains_fleet_image_in_lds(const NetDesc &net)
{
  return wave_net_image_in_lds(net, kNgFixedFloats, kNgLdsLimit);
}

hipError_t launch_nominal_gains_fleet(const NominalGainsFleetArgs *h_inst, const NominalGainsFleetArgs *d_inst, int n, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  if (n > kMaxFleet) return hipErrorInvalidValue;
  size_t lds = sizeof(float) * (size_t)kNgFixedFloats;
  for (int i = 0; i < n; i++) {
    const NetDesc &net = h_inst[i].net;
    if (!wave_net_valid(net) || h_inst[i].T < 2) return hipErrorInvalidValue;
    if (h_inst[i].img_lds) {
      if (!nominal_gains_fleet_image_in_lds(net)) return hipErrorInvalidValue;
      lds = std::max(lds, sizeof(float) * ((size_t)kNgFixedFloats + (size_t)net.num_params));
    }
  }
  if (hipError_t e = raise_lds_limit_once<nominal_gains_fleet_kernel>(kNgLdsLimit); e != hipSuccess) return e;
  hipLaunchKernelGGL(nominal_gains_fleet_kernel, dim3(n), dim3(64 * kDdpFleetWaves), lds, stream, d_inst);
  return hipGetLastError();
}

}  // namespace mppi
