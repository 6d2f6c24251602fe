// rollout_row.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) for gfx950, the LATENCY form of 32-wide nets:
// the network on the VECTOR ALU, four rollouts per dynamics wavefront, four dynamics wavefronts + the four riders of
// group_roles.hpp (pose -> cost, noise -> control) per 16 rollouts.  Used while every group has a CU of its own
// (K <= 16 x #CUs: BASELINE configs 1-3, the reference's K = 1920).
//
// Why not the matrix instruction here: at one group per CU the T-step recurrence is a latency chain, and a dependent
// k-step of v_mfma_f32_16x16x4_f32 costs ~8 cycles (4 k per 32-cycle instruction), so a 32-input layer
// is 8 x 33 = 264 cycles on top of a hand-over between the two waves that share the layer (the quad form: ~1 530
// cycles per step).  A dependent v_pk_fma_f32 issues every ~9 cycles too but carries TWO neurons and needs no partner:
//   * one dynamics wave = 4 rollouts x 16 lanes = 4 DPP ROWS; lane (r, p) owns neurons 2p, 2p+1 of every hidden layer of
//     rollout r (outputs 2(p&1), 2(p&1)+1 of the last layer), their weights in registers as pairs;
//   * a layer = per lane the k-ascending fmaf chain of mppi_controller.cu's dot product (neural_net_model.cu:379-394;
//     bias afterwards) -- bit-identical to every other form -- with the activation a_k broadcast to both halves of the
//     packed multiply-add (op_sel);
//   * the activations of a layer never leave the registers: `row_newbcast:q` of the DPP hands every lane of a row the
//     value of lane q, one v_mov_b64_dpp per PAIR of k (round 4; one v_mov_b32_dpp per k before), issued in the shadow of
//     the multiply-adds (round 3, second half;
//     before that a layer's activations went through LDS -- one 8-B write and eight 16-B broadcast reads per lane and layer:
//     tools/ub/row_bcast_ub.hip measures the recurrence alone on a SIMD at 865 cycles per step against 1 120).  No other
//     wave is involved: no sequence word, no poll, no barrier on the recurrence;
//   * lanes 0 and 1 of a row hold the state pair (s3, s4) / (s5, s6) (every even / odd lane computes the same two
//     outputs), so layer 0 of the next step reads the new state through four of the same moves;
//   * state records, controls, texels, noise: the rings and riders of group_roles.hpp, one rider per SIMD beside one
//     dynamics wave.  The riders work in chunks of four steps, so the dynamics waves hand over per chunk too: one sequence
//     word and one look at the control wave's count per four steps, ring slots as instruction offsets (row_step,
//     row_dynamics: the invariants are written down there).
#include "group_roles.hpp"
#include "mppi_kernels.hpp"

namespace mppi {

// Diagnostic build only (-DMPPI_ROW_STAMPS, tools/row_stamps.py): s_memtime stamps of workgroup 0 -- where the time of a
// launch goes outside the T loop.  The product build has no stamp instruction.
#ifdef MPPI_ROW_STAMPS
__device__ unsigned long long g_row_stamps[16];
#define RSTAMP(i)                                                                                         \
  do {                                                                                                    \
    if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) {                                                     \
      unsigned long long t__;                                                                             \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)::"memory");                           \
      g_row_stamps[i] = t__;                                                                              \
    }                                                                                                     \
  } while (0)
#endif

}  // namespace mppi

// the group itself -- shared state, weights in registers, row_dot_bc, row_out_tree, row_step, row_dynamics, row_group -- is
// row_group.hpp's, shared with rollout_row32.hip; the kernels of this file are its NHH = 1 (one hidden-to-hidden layer)
#include "row_group.hpp"

namespace mppi {

template <int H, bool AFFINE, bool CTRL, bool TREE>
__global__ __launch_bounds__(512) void rollout_row_kernel(const RolloutArgs a)
{
  __shared__ __attribute__((aligned(16))) RowShared<H> sh;
  row_group<H, 1, AFFINE, CTRL, TREE>(a, sh);
}
// the same kernel enqueued one solve ahead (a.gate != nullptr): see group_gate_wait (mppi_device.hpp)
template <int H, bool AFFINE, bool CTRL, bool TREE>
__global__ __launch_bounds__(512) void rollout_row_gated_kernel(const RolloutArgs a)
{
  __shared__ __attribute__((aligned(16))) RowShared<H> sh;
  row_group<H, 1, AFFINE, CTRL, TREE, true>(a, sh);
}

// several instances in one launch (mppi_compute_control_batch): grid (groups of the largest instance, instances) -- workgroup
// (x, y) runs group x of instance y, whose argument block sits at a position the workgroup knows from its own index
// (MPPI_BATCH_DISPATCH, mppi_device.hpp: one branch per instance, so that the block is read as the single-instance kernel
// reads its arguments -- with a run-time index the block went through scratch: 44.8 us beside 33.8 us alone)
template <int H, bool AFFINE, bool CTRL, bool TREE, int NB>
__global__ __launch_bounds__(512) void rollout_row_batch_kernel(const QuadBatchArgsT<NB> b)
{
  __shared__ __attribute__((aligned(16))) RowShared<H> sh;
#define MPPI_ROW_BODY(A)                                                                                   \
  do {                                                                                                     \
    if ((int)blockIdx.x >= (A).K / kRolloutsPerWave) return; /* a smaller instance than the largest */     \
    row_group<H, 1, AFFINE, CTRL, TREE>((A), sh);                                                          \
  } while (0)
  MPPI_BATCH_DISPATCH(NB, b, MPPI_ROW_BODY);
#undef MPPI_ROW_BODY
}

// the same batched kernel enqueued one solve ahead (mppi_arm_batch): every instance's argument block carries its OWN handle's
// gate block (a.gate, a.gate_seq, a.gate_ticks; a.U points at the nominal sequence inside it), whose pose wave polls replica
// blockIdx.x % kGateReplicas of it -- blockIdx.x is the group index inside the instance, as in the single gated kernel
template <int H, bool AFFINE, bool CTRL, bool TREE, int NB>
__global__ __launch_bounds__(512) void rollout_row_batch_gated_kernel(const QuadBatchArgsT<NB> b)
{
  __shared__ __attribute__((aligned(16))) RowShared<H> sh;
#define MPPI_ROW_BODY(A)                                                                                   \
  do {                                                                                                     \
    if ((int)blockIdx.x >= (A).K / kRolloutsPerWave) return; /* a smaller instance than the largest */     \
    row_group<H, 1, AFFINE, CTRL, TREE, true>((A), sh);                                                    \
  } while (0)
  MPPI_BATCH_DISPATCH(NB, b, MPPI_ROW_BODY);
#undef MPPI_ROW_BODY
}

bool row_variant_supported(int hidden, int n_hidden) { return hidden == 32 && n_hidden == 2; }
int row_pack_floats() { return row_pack_layout(1).entries * 16 * 4; }

// The four (AFFINE, CTRL) instances of a kernel template, tree or exact
#define MPPI_ROW_DISPATCH(LAUNCH, KERN, TREE, ...)                                                            \
  do {                                                                                                        \
    if (affine && !ctrl) LAUNCH((KERN<32, true, false, TREE>), __VA_ARGS__);                                  \
    else if (affine && ctrl) LAUNCH((KERN<32, true, true, TREE>), __VA_ARGS__);                               \
    else if (!affine && !ctrl) LAUNCH((KERN<32, false, false, TREE>), __VA_ARGS__);                           \
    else LAUNCH((KERN<32, false, true, TREE>), __VA_ARGS__);                                                  \
  } while (0)
#define MPPI_ROW_BATCH_DISPATCH(KERN, TREE, NB, ...)                                                                            \
  do {                                                                                                                          \
    if (affine && !ctrl) hipLaunchKernelGGL((KERN<32, true, false, TREE, NB>), __VA_ARGS__);                                    \
    else if (affine && ctrl) hipLaunchKernelGGL((KERN<32, true, true, TREE, NB>), __VA_ARGS__);                                 \
    else if (!affine && !ctrl) hipLaunchKernelGGL((KERN<32, false, false, TREE, NB>), __VA_ARGS__);                             \
    else hipLaunchKernelGGL((KERN<32, false, true, TREE, NB>), __VA_ARGS__);                                                    \
  } while (0)

hipError_t launch_rollout_row_batch(const QuadBatchArgs &b, bool tree, hipStream_t stream)
{
  if (b.n < 1 || b.n > kMaxBatch) return hipErrorInvalidValue;
  bool affine = true, ctrl = false;  // the general forms are exact supersets (rollout_mfma.hip)
  int gmax = 0;
  const bool gated = b.inst[0].gate != nullptr;  // mppi_arm_batch: every instance gated on its own block, or none
  for (int i = 0; i < b.n; i++) {
    if ((b.inst[i].gate != nullptr) != gated) return hipErrorInvalidValue;
    affine = affine && b.inst[i].cost.affine != 0;
    ctrl = ctrl || b.inst[i].cost.need_control_cost != 0;
    gmax = b.inst[i].K / kRolloutsPerWave > gmax ? b.inst[i].K / kRolloutsPerWave : gmax;
  }
  const dim3 grid(gmax, b.n), block(512);
  if (b.n <= 2) {  // the two controllers of a tick: half the argument segment
    const QuadBatchArgsT<2> b2 = batch_args_prefix<2>(b);
    if (gated) {
      if (tree) MPPI_ROW_BATCH_DISPATCH(rollout_row_batch_gated_kernel, true, 2, grid, block, 0, stream, b2);
      else MPPI_ROW_BATCH_DISPATCH(rollout_row_batch_gated_kernel, false, 2, grid, block, 0, stream, b2);
    } else {
      if (tree) MPPI_ROW_BATCH_DISPATCH(rollout_row_batch_kernel, true, 2, grid, block, 0, stream, b2);
      else MPPI_ROW_BATCH_DISPATCH(rollout_row_batch_kernel, false, 2, grid, block, 0, stream, b2);
    }
  } else {
    if (gated) {
      if (tree) MPPI_ROW_BATCH_DISPATCH(rollout_row_batch_gated_kernel, true, 4, grid, block, 0, stream, b);
      else MPPI_ROW_BATCH_DISPATCH(rollout_row_batch_gated_kernel, false, 4, grid, block, 0, stream, b);
    } else {
      if (tree) MPPI_ROW_BATCH_DISPATCH(rollout_row_batch_kernel, true, 4, grid, block, 0, stream, b);
      else MPPI_ROW_BATCH_DISPATCH(rollout_row_batch_kernel, false, 4, grid, block, 0, stream, b);
    }
  }
  return hipGetLastError();
}

hipError_t launch_rollout_row(int hidden, int n_hidden, const RolloutArgs &a, bool tree, hipStream_t stream)
{
  if (!row_variant_supported(hidden, n_hidden) || a.K % kRolloutsPerWave != 0) return hipErrorInvalidValue;
  const bool affine = a.cost.affine != 0, ctrl = a.cost.need_control_cost != 0;
  const dim3 grid(a.K / kRolloutsPerWave), block(512);
  if (a.gate != nullptr) {
    if (tree) MPPI_ROW_DISPATCH(MPPI_LAUNCH_ROLLOUT, rollout_row_gated_kernel, true, grid, block, 0, stream, a);
    else MPPI_ROW_DISPATCH(MPPI_LAUNCH_ROLLOUT, rollout_row_gated_kernel, false, grid, block, 0, stream, a);
    return hipGetLastError();
  }
  if (tree) MPPI_ROW_DISPATCH(MPPI_LAUNCH_ROLLOUT, rollout_row_kernel, true, grid, block, 0, stream, a);
  else MPPI_ROW_DISPATCH(MPPI_LAUNCH_ROLLOUT, rollout_row_kernel, false, grid, block, 0, stream, a);
  return hipGetLastError();
}
#undef MPPI_ROW_DISPATCH
#undef MPPI_ROW_BATCH_DISPATCH

}  // namespace mppi

#ifdef MPPI_ROW_STAMPS
extern "C" int mppi_debug_read_row_stamps(unsigned long long *out)
{
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mppi::g_row_stamps), sizeof(unsigned long long) * 16);
}
#endif
