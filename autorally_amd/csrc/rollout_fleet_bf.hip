// rollout_fleet_bf.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) for gfx950 with the basis-function model
// (GeneralizedLinear<CarBasisFuncs,...>), the workgroups of rollout_bf.hip (bf_group.hpp: one, two or three waves per 64
// rollouts) for a FLEET of up to kMaxFleet independent controllers in ONE launch.  Grid (64-rollout groups of the largest
// instance, instances); workgroup (x, y) runs group x of inst[y], where inst is an array of argument blocks in DEVICE MEMORY,
// read exactly as rollout_fleet_multi_kernel reads its own: the index is workgroup-uniform and the array read-only behind a
// __restrict__ pointer, so the block arrives in scalar registers as a kernel argument does (profiles/r28_a_fleet_bf_isa.txt).  A
// workgroup beyond its instance's K leaves before it touches LDS or the barrier.  Eps comes from the instance's noise buffer
// (the fleet's generator launch or the caller's explicit noise), never from the control wave's generator; not gated.  The step is
// bf_group.hpp's, unchanged: the bits of "bf3", whatever the wave count.
#include "bf_group.hpp"

namespace mppi {

// The plan of a launch: the wave count form_of (abi_forms.hip) chooses for one handle, with the groups counted over the fleet --
// three waves per group while every wave of every group gets a SIMD of its own, two while every group's two do on twice the
// SIMDs' slots (G <= simds), else one; forced_waves 1..3 overrides it.  Grid x = the groups of the largest instance, grid y = the
// instances.  All zero for n outside 1..kMaxFleet, a K that is no whole number of groups or a forced_waves outside 0..3.
FleetBfPlan fleet_bf_plan(const int *Ks, int n, int simds, int forced_waves)
{
  FleetBfPlan p{};
  if (!Ks || n < 1 || n > kMaxFleet || forced_waves < 0 || forced_waves > 3) return p;
  int kmax = 0;
  long groups = 0;
  for (int i = 0; i < n; i++) {
    if (Ks[i] < 64 || Ks[i] % 64 != 0) return p;
    kmax = Ks[i] > kmax ? Ks[i] : kmax;
    groups += Ks[i] / 64;
  }
  p.waves = forced_waves ? forced_waves : (3 * groups <= simds ? 3 : (groups <= simds ? 2 : 1));
  p.threads = 64 * p.waves;
  p.grid_x = kmax / 64;
  p.grid_y = n;
  return p;
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * kBfLanes) void rollout_fleet_bf_kernel(const RolloutArgs *__restrict__ inst, const int n)
{
  if ((int)blockIdx.y >= n) return;
  RolloutArgs a = inst[blockIdx.y];  // workgroup-uniform, read-only: scalar loads
  // the pointers it holds are global memory, as those of a kernel argument are known to be
  a.U = load_global_ptr(inst[blockIdx.y].U);
  a.noise = load_global_ptr(inst[blockIdx.y].noise);
  a.costs = load_global_ptr(inst[blockIdx.y].costs);
  a.wpack = load_global_ptr(inst[blockIdx.y].wpack);
  a.inv_t = load_global_ptr(inst[blockIdx.y].inv_t);
  a.rng_in = load_global_ptr(inst[blockIdx.y].rng_in);
  a.rng_out = load_global_ptr(inst[blockIdx.y].rng_out);
  a.gate = load_global_ptr(inst[blockIdx.y].gate);
  a.min_cost = load_global_ptr(inst[blockIdx.y].min_cost);
  a.cost.map = load_global_ptr(inst[blockIdx.y].cost.map);
  // no group of this instance (a smaller K than the largest): nothing in LDS, no barrier
  if (64 * (int)blockIdx.x >= a.K) return;
  if constexpr (WAVES == 3) bf3_group(a, (int)blockIdx.x);
  else if constexpr (WAVES == 2) bf2_group(a, (int)blockIdx.x);
  else bf1_group(a, (int)blockIdx.x);
}

// h_inst: the host's copy of the n argument blocks (the plan is read from it); d_inst: the same blocks in device memory,
// complete once `stream` reaches the launch.  Every instance: eps in its noise buffer, not gated.  (Affine costmap transform and
// control cost are run-time flags of these workgroups; which sets share a launch is abi_solve.hip's fleet_together.)
hipError_t launch_rollout_fleet_bf(const RolloutArgs *h_inst, const RolloutArgs *d_inst, int n, int simds, int forced_waves, hipStream_t stream)
{
  if (!h_inst || !d_inst || n < 1 || n > kMaxFleet) return hipErrorInvalidValue;
  int Ks[kMaxFleet];
  for (int i = 0; i < n; i++) {
    if (h_inst[i].gate != nullptr || h_inst[i].inline_noise != 0) return hipErrorInvalidValue;
    Ks[i] = h_inst[i].K;
  }
  const FleetBfPlan p = fleet_bf_plan(Ks, n, simds, forced_waves);
  if (p.threads == 0) return hipErrorInvalidValue;
  const dim3 grid(p.grid_x, p.grid_y), block(p.threads);
  if (p.waves == 3) MPPI_LAUNCH_ROLLOUT(rollout_fleet_bf_kernel<3>, grid, block, 0, stream, d_inst, n);
  else if (p.waves == 2) MPPI_LAUNCH_ROLLOUT(rollout_fleet_bf_kernel<2>, grid, block, 0, stream, d_inst, n);
  else MPPI_LAUNCH_ROLLOUT(rollout_fleet_bf_kernel<1>, grid, block, 0, stream, d_inst, n);
  return hipGetLastError();
}

}  // namespace mppi
