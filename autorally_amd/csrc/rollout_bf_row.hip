// rollout_bf_row.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) with the basis-function dynamics
// (GeneralizedLinear<CarBasisFuncs,7,2,25,...>, PI/generalized_linear.cu:169-245, PI/car_bfs.cuh:44-120) in the LATENCY
// layout of rollout_row.hip: 16 rollouts per workgroup, four dynamics wavefronts of four rollouts each and the four riders of
// group_roles.hpp (noise -> control, pose -> cost).  "bf_row", by name only.
//
// The reference runs the model with BLOCKSIZE_Y = 4 threads per rollout: for each of the four outputs, y-thread y sums the
// basis functions i = y, y + 4, ... and the four partial sums are added (basis_dynamics, basis_funcs.hpp: in the order
// y = 0, 1, 2, 3).  That is sixteen (output, y-thread) cells per rollout -- one DPP row:
//   * lane 16 r + 4 j + y of dynamics wave w serves rollout 4 w + r of the group, output j (state component s[3 + j]) and
//     y-thread y; its <= 7 weights W[j][y + 4 m], the divisors of its <= 7 basis functions with their reciprocals and a mark on
//     each (plain value / quotient / zero below the u_x switch / the double quotient) come from the image pack_bf_row_weights
//     writes (abi_pack.hip), 96 B per lane;
//   * every lane evaluates the shared sub-expressions (basis_shared_fast: one instruction serves 64 lanes as it serves 4) and
//     the ~20 plain products the numerators are made of, selects ITS numerators by y, runs its <= 7 independent Markstein
//     quotients (div_const) and its one chain part = fmaf(W, phi, part), m ascending from part = 0: the operations of
//     basis_funcs_from and basis_dynamics_dev (bf_device.hpp) on the same operands in the same order, hence their bits;
//   * the four partials of a quad are added in the order y = 0, 1, 2, 3 from +0 (quad_perm moves), every lane of quad j then
//     holds d[j] and updates s[3 + j]; four row broadcasts hand every lane the new s3..s6;
//   * lanes y = 0 write the step's record rec[slot][rollout][j]; the other lanes' copy goes to a dump word nobody reads (no exec
//     masking on the recurrence).  One sequence word per step (NSW = 1, published behind every record).
// x, y, yaw, the costmap fetches, the cost and the controls are the riders' work: the pose wave's kinematics with
// a.negate_yaw_der = 1 (the launcher's side: abi_solve.hip) are computeKinematics of generalized_linear.cu:212-217.
// Results are bit for bit those of rollout_bf.hip's kernels.
#include "bf_row_device.hpp"

namespace mppi {

struct BfRowShared {
  static constexpr int NW = 4;             // dynamics waves per group, four rollouts each
  static constexpr int NSW = 1;            // xseq[w] = steps published by dynamics wave w
  static constexpr bool kRecByAll = true;  // every dynamics wave writes the state records of its own rollouts
  static constexpr int kR = 16;            // rollouts per group
  int xseq[NW][64];
  float rec[kGRing][kRolloutsPerWave][4];  // s3..s6 before the update of step t
  int cost_done[64];
  float ctl_b1[kGRing][64];
  float ctl_rec[kGRing][kRolloutsPerWave][4];
  int ctl_pub[64];
  float tex[kGRing][kRolloutsPerWave][2];
  int pose_pub[64];
  float eps[kGRing][kRolloutsPerWave][2];
  int rng_pub[64];
  int fail[4];
  int fin[8];
  float gstate[8];  // gated launch: the vehicle state the pose wave took from the gate block, then 1 in gate_open[]
  int gate_open[8];
  float dump[NW][64];  // where lanes y != 0 of a dynamics wave put their copy of the state component (never read)
};

// The dynamics wave w of a group: T - 1 steps, the state record of every step.  Hand-over with the riders (group_roles.hpp),
// one sequence word per step:
//   * xseq[w] = t + 1 is published behind the record of step t; the controls of step t were read before it (the control wave
//     reuses a ring slot once every dynamics wave has published the step that used it);
//   * step t + 1 starts when the control wave has published it; that also says its record's ring slot is free (the control wave
//     publishes a chunk that ends with step tm only after the cost wave has consumed step tm - kGRing, group_control_wave);
//   * the control wave's count and the controls of step t + 1 are requested at the start of step t and tested at its end: the
//     control wave runs ahead, so the (cold) poll behind the step is the exception;
//   * every poll is one unit of the wave's budget; a wave without budget stops waiting, runs to its end and raises fail.
template <bool GATED>
__device__ __forceinline__ void bf_row_dynamics(const RolloutArgs &a, BfRowShared &sh, const int w)
{
  const int lane = threadIdx.x & 63;
  const int r = lane >> 4, p = lane & 15, j = p >> 2, y = p & 3;
  const int jr = 4 * w + r;  // rollout of the group
  const int T = a.T;
  BfRowLane L;
  bf_row_load(a.wpack, p, L);

  const uint32_t a_myseq = lds_addr(&sh.xseq[w][lane]);
  typedef const volatile int __attribute__((address_space(3))) *lds_int_p;
  typedef const volatile f32x2 __attribute__((address_space(3))) *lds_f2_p;
  const lds_int_p p_pub = (lds_int_p)&sh.ctl_pub[0];
  const lds_f2_p p_u = (lds_f2_p)&sh.ctl_rec[0][jr][0];  // clamped (u0, u1) of this lane's rollout, ring slot 0
  constexpr int kSlotF2 = kRolloutsPerWave * 2;          // f32x2 per ring slot of ctl_rec
  // record: lanes y = 0 into rec[slot][jr][j], the others into their dump word whatever the slot
  const uint32_t a_rec0 = (y == 0) ? lds_addr(&sh.rec[0][jr][j]) : lds_addr(&sh.dump[w][lane]);
  const uint32_t rec_stride = (y == 0) ? (uint32_t)(sizeof(float) * kRolloutsPerWave * 4) : 0u;

  int budget = spin_budget_init(a.spin_budget, T, a.fault_wave == w + 1);
  float s3, s4, s5, s6;
  if constexpr (GATED) {
    // the state arrives through the gate block: the pose wave has put it into LDS (the image above was loaded meanwhile)
    const uint32_t a_go = lds_addr(&sh.gate_open[0]);
    while (lds_peek(a_go) == 0 && --budget > 0) __builtin_amdgcn_s_sleep(1);
    const volatile float *gs = sh.gstate;
    s3 = gs[3]; s4 = gs[4]; s5 = gs[5]; s6 = gs[6];
  } else {
    s3 = a.state[3]; s4 = a.state[4]; s5 = a.state[5]; s6 = a.state[6];
  }
  float sj = bf_sel4(j, s3, s4, s5, s6);  // this quad's component
  int cp = 0;  // steps the control wave has published, as far as this wave knows
  while ((cp = __builtin_amdgcn_readfirstlane(*p_pub)) < 1 && --budget > 0) __builtin_amdgcn_s_sleep(1);
  f32x2 un = p_u[0];

  // Steps 0 .. T-2 in full; of step T-1 only the state record goes out (its update feeds nothing: the cost is the running mean
  // over the states BEFORE the updates of steps 1..T-1, mppi_controller.cu:160-177).
  for (int t = 0; t < T; t++) {
    const f32x2 u = un;
    asm volatile("ds_write_b32 %0, %1" ::"v"(a_rec0 + (uint32_t)(t & (kGRing - 1)) * rec_stride), "v"(sj) : "memory");
    lds_publish(a_myseq, t + 1);
    if (t == T - 1) break;
    // requested now, tested behind the step: the control wave's count, then the controls of step t + 1 (valid if the count
    // read before them is >= t + 2)
    const lds_f2_p pu = p_u + ((t + 1) & (kGRing - 1)) * kSlotF2;
    const int cp_v = *p_pub;
    un = *pu;
    const float d = bf_row_deriv(L, y, s3, s4, s5, s6, u.x, u.y);
    sj = fmaf(d, a.dt, sj);  // incrementState
    s3 = bf_row_bc<0>(sj); s4 = bf_row_bc<4>(sj); s5 = bf_row_bc<8>(sj); s6 = bf_row_bc<12>(sj);
    cp = __builtin_amdgcn_readfirstlane(cp_v);
    const int want = t + 2;
    if (__builtin_expect(cp < want, 0)) {
      while (cp < want && --budget > 0) {
        cp = __builtin_amdgcn_readfirstlane(*p_pub);
        un = *pu;
      }
    }
  }
  spin_finish(budget, lds_addr(&sh.fail[0]), lds_addr(&sh.fin[w]));
}

// one group (workgroup): the four dynamics waves and the four riders
template <bool AFFINE, bool CTRL, bool GATED>
__device__ __forceinline__ void bf_row_group(const RolloutArgs &a, BfRowShared &sh)
{
  using SH = BfRowShared;
  using R = GroupRoles<SH>;
  const int lane = threadIdx.x & 63;
  const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  MrgHalf g0{0, 0, 0};
  if (role == R::kRng) g0 = group_rng_load<SH>(a);  // in front of the barrier: the head of the launch's critical path
  if (role == 0) {  // sequence words start at 0; the only barrier
#pragma unroll
    for (int w = 0; w < SH::NW; w++) sh.xseq[w][lane] = 0;
    sh.cost_done[lane] = 0;
    sh.ctl_pub[lane] = 0;
    sh.pose_pub[lane] = 0;
    sh.rng_pub[lane] = 0;
    sh.fail[lane & 3] = 0;
    sh.fin[lane & 7] = 0;
    sh.gate_open[lane & 7] = 0;
  }
  __syncthreads();
  if (role < SH::NW) bf_row_dynamics<GATED>(a, sh, role);
  else if (role == R::kCost) group_cost_wave4<SH, CTRL>(a, sh);
  else if (role == R::kCtl) group_control_wave(a, sh, GATED ? lds_addr(&sh.gate_open[0]) : 0u);
  else if (role == R::kPose) {
    if constexpr (GATED) {
      const int shut = group_gate_wait(a, sh);
      const volatile float *gs = sh.gstate;
      const float x0 = gs[0], y0 = gs[1], yaw0 = gs[2];
      group_pose_wave4<SH, AFFINE>(a, sh, x0, y0, yaw0, shut);
    } else {
      group_pose_wave4<SH, AFFINE>(a, sh);
    }
  }
  else group_rng_wave<SH, true>(a, sh, g0);
}

template <bool AFFINE, bool CTRL>
__global__ __launch_bounds__(512) void rollout_bf_row_kernel(const RolloutArgs a)
{
  __shared__ __attribute__((aligned(16))) BfRowShared sh;
  bf_row_group<AFFINE, CTRL, false>(a, sh);
}
// the same kernel enqueued one solve ahead (a.gate != nullptr): see group_gate_wait (mppi_device.hpp)
template <bool AFFINE, bool CTRL>
__global__ __launch_bounds__(512) void rollout_bf_row_gated_kernel(const RolloutArgs a)
{
  __shared__ __attribute__((aligned(16))) BfRowShared sh;
  bf_row_group<AFFINE, CTRL, true>(a, sh);
}

// several instances in one launch (mppi_compute_control_batch, mppi_arm_batch): grid (groups of the largest instance,
// instances), the instance's argument block at a compile-time position (MPPI_BATCH_DISPATCH, mppi_device.hpp)
template <bool AFFINE, bool CTRL, int NB>
__global__ __launch_bounds__(512) void rollout_bf_row_batch_kernel(const QuadBatchArgsT<NB> b)
{
  __shared__ __attribute__((aligned(16))) BfRowShared sh;
#define MPPI_BF_ROW_BODY(A)                                                                                \
  do {                                                                                                     \
    if ((int)blockIdx.x >= (A).K / kRolloutsPerWave) return; /* a smaller instance than the largest */     \
    bf_row_group<AFFINE, CTRL, false>((A), sh);                                                            \
  } while (0)
  MPPI_BATCH_DISPATCH(NB, b, MPPI_BF_ROW_BODY);
#undef MPPI_BF_ROW_BODY
}
template <bool AFFINE, bool CTRL, int NB>
__global__ __launch_bounds__(512) void rollout_bf_row_batch_gated_kernel(const QuadBatchArgsT<NB> b)
{
  __shared__ __attribute__((aligned(16))) BfRowShared sh;
#define MPPI_BF_ROW_BODY(A)                                                                                \
  do {                                                                                                     \
    if ((int)blockIdx.x >= (A).K / kRolloutsPerWave) return; /* a smaller instance than the largest */     \
    bf_row_group<AFFINE, CTRL, true>((A), sh);                                                             \
  } while (0)
  MPPI_BATCH_DISPATCH(NB, b, MPPI_BF_ROW_BODY);
#undef MPPI_BF_ROW_BODY
}

int bf_row_pack_floats() { return kBfRowPackEntries * 16 * 4; }

#define MPPI_BF_ROW_DISPATCH(LAUNCH, KERN, ...)                                  \
  do {                                                                           \
    if (affine && !ctrl) LAUNCH((KERN<true, false>), __VA_ARGS__);               \
    else if (affine && ctrl) LAUNCH((KERN<true, true>), __VA_ARGS__);            \
    else if (!affine && !ctrl) LAUNCH((KERN<false, false>), __VA_ARGS__);        \
    else LAUNCH((KERN<false, true>), __VA_ARGS__);                               \
  } while (0)
#define MPPI_BF_ROW_BATCH_DISPATCH(KERN, ...)                                                   \
  do {                                                                                          \
    if (affine && !ctrl) hipLaunchKernelGGL((KERN<true, false, 2>), __VA_ARGS__);               \
    else if (affine && ctrl) hipLaunchKernelGGL((KERN<true, true, 2>), __VA_ARGS__);            \
    else if (!affine && !ctrl) hipLaunchKernelGGL((KERN<false, false, 2>), __VA_ARGS__);        \
    else hipLaunchKernelGGL((KERN<false, true, 2>), __VA_ARGS__);                               \
  } while (0)

hipError_t launch_rollout_bf_row(const RolloutArgs &a, hipStream_t stream)
{
  if (a.K % kRolloutsPerWave != 0) return hipErrorInvalidValue;
  const bool affine = a.cost.affine != 0, ctrl = a.cost.need_control_cost != 0;
  const dim3 grid(a.K / kRolloutsPerWave), block(512);
  if (a.gate != nullptr) MPPI_BF_ROW_DISPATCH(MPPI_LAUNCH_ROLLOUT, rollout_bf_row_gated_kernel, grid, block, 0, stream, a);
  else MPPI_BF_ROW_DISPATCH(MPPI_LAUNCH_ROLLOUT, rollout_bf_row_kernel, grid, block, 0, stream, a);
  return hipGetLastError();
}

// the two controllers of a tick in one launch (the batched kernels exist for two instances)
hipError_t launch_rollout_bf_row_batch(const QuadBatchArgs &b, hipStream_t stream)
{
  if (b.n != 2) return hipErrorInvalidValue;
  bool affine = true, ctrl = false;  // the instances agree on both (abi_solve.hip: batch_together)
  int gmax = 0;
  const bool gated = b.inst[0].gate != nullptr;  // mppi_arm_batch: every instance gated on its own block, or none
  for (int i = 0; i < b.n; i++) {
    if ((b.inst[i].gate != nullptr) != gated) return hipErrorInvalidValue;
    affine = affine && b.inst[i].cost.affine != 0;
    ctrl = ctrl || b.inst[i].cost.need_control_cost != 0;
    gmax = b.inst[i].K / kRolloutsPerWave > gmax ? b.inst[i].K / kRolloutsPerWave : gmax;
  }
  const dim3 grid(gmax, b.n), block(512);
  const QuadBatchArgsT<2> b2 = batch_args_prefix<2>(b);
  if (gated) MPPI_BF_ROW_BATCH_DISPATCH(rollout_bf_row_batch_gated_kernel, grid, block, 0, stream, b2);
  else MPPI_BF_ROW_BATCH_DISPATCH(rollout_bf_row_batch_kernel, grid, block, 0, stream, b2);
  return hipGetLastError();
}
#undef MPPI_BF_ROW_DISPATCH
#undef MPPI_BF_ROW_BATCH_DISPATCH

}  // namespace mppi
