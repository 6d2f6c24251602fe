// rollout_fleet_multi.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) for gfx950, the workgroup of "multi4_tree_gen"
// (multi_group.hpp: four dynamics waves with every weight in registers, the riders pose | fetch | cost, a control wave, the
// output layer as a butterfly, eps from the stand-alone generator, not gated) for a FLEET of up to kMaxFleet independent
// controllers of one standard network in ONE launch.  Grid (64-rollout groups of the largest instance, instances); workgroup
// (x, y) runs group x of inst[y], where inst is an array of argument blocks in DEVICE MEMORY, read exactly as
// rollout_fleet16_kernel reads its own: the index is workgroup-uniform and the array read-only behind a __restrict__ pointer,
// so the block arrives in scalar registers as a kernel argument does (profiles/r24_a_fleet_multi4_isa.txt).  A workgroup
// beyond its instance's K leaves before it touches LDS or the barrier.  The step is multi_group's, unchanged: the bits of
// "multi4_tree_gen".
#include "multi_group.hpp"

namespace mppi {

// The plan of a launch: eight waves per workgroup of 64 rollouts, grid x = the groups of the largest instance, grid y = the
// instances.  All zero for a shape the multi form does not have, n outside 1..kMaxFleet or a K that is no whole number of groups.
FleetMultiPlan fleet_multi_plan(int hidden, int n_hidden, const int *Ks, int n)
{
  FleetMultiPlan p{};
  if (!multi_variant_supported(hidden, n_hidden) || !Ks || n < 1 || n > kMaxFleet) return p;
  int kmax = 0;
  for (int i = 0; i < n; i++) {
    if (Ks[i] < 64 || Ks[i] % 64 != 0) return p;
    kmax = Ks[i] > kmax ? Ks[i] : kmax;
  }
  p.threads = 8 * 64;
  p.grid_x = kmax / 64;
  p.grid_y = n;
  return p;
}

template <int H, int NHID>
__global__ __launch_bounds__(8 * 64, 1) void rollout_fleet_multi_kernel(const RolloutArgs *__restrict__ inst, const int n)
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
  multi_group<H, NHID, 4, true, true, false, true>(a, (int)blockIdx.x);
}

// h_inst: the host's copy of the n argument blocks (the plan is read from it); d_inst: the same blocks in device memory,
// complete once `stream` reaches the launch.  Every instance: one shape, eps in its noise buffer, not gated.  (Affine costmap
// transform and control cost are run-time flags of the multi form: the instances of a launch may differ in them as far as the
// kernel goes; which sets share a launch is abi_solve.hip's fleet_together.)
hipError_t launch_rollout_fleet_multi(int hidden, int n_hidden, const RolloutArgs *h_inst, const RolloutArgs *d_inst, int n, hipStream_t stream)
{
  if (!h_inst || !d_inst || n < 1 || n > kMaxFleet) return hipErrorInvalidValue;
  int Ks[kMaxFleet];
  for (int i = 0; i < n; i++) {
    if (h_inst[i].gate != nullptr || h_inst[i].inline_noise != 0) return hipErrorInvalidValue;
    Ks[i] = h_inst[i].K;
  }
  const FleetMultiPlan p = fleet_multi_plan(hidden, n_hidden, Ks, n);
  if (p.threads == 0) return hipErrorInvalidValue;
  const dim3 grid(p.grid_x, p.grid_y), block(p.threads);
  if (hidden == 32 && n_hidden == 2) MPPI_LAUNCH_ROLLOUT((rollout_fleet_multi_kernel<32, 2>), grid, block, 0, stream, d_inst, n);
  else if (hidden == 64 && n_hidden == 2) MPPI_LAUNCH_ROLLOUT((rollout_fleet_multi_kernel<64, 2>), grid, block, 0, stream, d_inst, n);
  else if (hidden == 32 && n_hidden == 4) MPPI_LAUNCH_ROLLOUT((rollout_fleet_multi_kernel<32, 4>), grid, block, 0, stream, d_inst, n);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace mppi
