// mppi_kernels.hpp -- launchers implemented in the .hip kernel files.
#pragma once
#include "mppi_device.hpp"

#include <hip/hip_ext.h>
#include <atomic>
#include <type_traits>

namespace mppi {

// Rollout kernels are launched through this macro.  When the caller has set the two thread-local events
// (mppi_enable_stage_timing: the stage-timing pass of bench.py), the launch goes through
// hipExtLaunchKernelGGL, which stamps them with the begin / end of THIS kernel's dispatch -- the figure
// rocprofv3 --kernel-trace reports -- instead of the time between two marker packets around it (which on this
// runtime is 3-4 us longer).  Otherwise a plain launch.
extern thread_local hipEvent_t tl_kernel_start, tl_kernel_stop;
#define MPPI_LAUNCH_ROLLOUT(kern, grid, block, lds, stream, ...)                                                   \
  do {                                                                                                             \
    if (::mppi::tl_kernel_start != nullptr)                                                                        \
      hipExtLaunchKernelGGL(kern, grid, block, lds, stream, ::mppi::tl_kernel_start, ::mppi::tl_kernel_stop, 0,    \
                            __VA_ARGS__);                                                                          \
    else                                                                                                           \
      hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);                                             \
  } while (0)

// The launchers' run-time flags as compile-time ones: f(std::bool_constant<AFFINE>, std::bool_constant<CTRL>) -- and
// std::bool_constant<GATED> for the forms that have a gated kernel -- launches that instance and returns its hipError_t.
template <class F>
inline hipError_t dispatch_cost_flags(bool affine, bool ctrl, F &&f)
{
  if (affine && !ctrl) return f(std::true_type{}, std::false_type{});
  if (affine && ctrl) return f(std::true_type{}, std::true_type{});
  if (!affine && !ctrl) return f(std::false_type{}, std::false_type{});
  return f(std::false_type{}, std::true_type{});
}
template <class F>
inline hipError_t dispatch_rollout_flags(bool affine, bool ctrl, bool gated, F &&f)
{
  if (gated) return dispatch_cost_flags(affine, ctrl, [&](auto af, auto ct) { return f(af, ct, std::true_type{}); });
  return dispatch_cost_flags(affine, ctrl, [&](auto af, auto ct) { return f(af, ct, std::false_type{}); });
}

// More dynamic LDS than the default limit for kernel instance KERN: set once per instance and device.  The flag is atomic: some
// launchers are called from the host helper thread as well (abi_host.hip).
template <auto KERN>
inline hipError_t raise_lds_limit_once(size_t bytes)
{
  static std::atomic<bool> attr_set[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (!attr_set[dev].load(std::memory_order_acquire)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    attr_set[dev].store(true, std::memory_order_release);
  }
  return hipSuccess;
}

// What one launch for the instances of a batch needs: the cost flags that serve all of them (the general forms are exact
// supersets, rollout_mfma.hip), gated (mppi_arm_batch: every instance gated on its own block, or none) and the groups of the
// largest instance.  False for a mixed gated / ungated batch or a K that is no whole number of groups.
struct BatchFlags {
  bool affine = true, ctrl = false, gated = false;
  int gmax = 0;
};
inline bool batch_flags_of(const QuadBatchArgs &b, BatchFlags &f)
{
  f = BatchFlags{};
  f.gated = b.inst[0].gate != nullptr;
  for (int i = 0; i < b.n; i++) {
    if ((b.inst[i].gate != nullptr) != f.gated || b.inst[i].K % kRolloutsPerWave != 0) return false;
    f.affine = f.affine && b.inst[i].cost.affine != 0;
    f.ctrl = f.ctrl || b.inst[i].cost.need_control_cost != 0;
    f.gmax = b.inst[i].K / kRolloutsPerWave > f.gmax ? b.inst[i].K / kRolloutsPerWave : f.gmax;
  }
  return true;
}

// rollout_mfma.hip
bool mfma_variant_supported(int hidden, int n_hidden);
int mfma_pack_floats_per_lane(int hidden, int n_hidden);
hipError_t launch_rollout_mfma(int hidden, int n_hidden, const RolloutArgs &a, int block_threads,
                               hipStream_t stream);
// several instances in one launch of the quad form (every instance: 6 -> hidden x n_hidden -> 4)
hipError_t launch_rollout_quad_batch(int hidden, int n_hidden, const QuadBatchArgs &b, hipStream_t stream);
hipError_t launch_dynamics_mfma(int hidden, int n_hidden, const float *wpack, const float *states,
                                const float *controls, float *ders, int n, int negate_yaw_der,
                                hipStream_t stream);

// rollout_multi.hip: nd dynamics waves (16 rollouts each) + cost wave + control wave per workgroup, nd in {1, 2, 4}
bool multi_variant_supported(int hidden, int n_hidden);
hipError_t launch_rollout_multi(int hidden, int n_hidden, const RolloutArgs &a, int nd, hipStream_t stream);

// rollout_oct.hip: four dynamics waves (one M tile of a 64-wide net each) + pose, cost, control and noise wave per
// 16 rollouts
bool oct_variant_supported(int hidden, int n_hidden);
hipError_t launch_rollout_oct(int hidden, int n_hidden, const RolloutArgs &a, hipStream_t stream);

// rollout_row.hip: latency form of 6-32-32-4 on the vector ALU -- four dynamics waves (four rollouts each) + pose, cost,
// control and noise wave per 16 rollouts; a.wpack = the weights in register order (pack_row_weights, mppi_abi.hip)
bool row_variant_supported(int hidden, int n_hidden);
int row_pack_floats();
// tree: the output layer as own-activation partials + a DPP butterfly (NOT the reference's summation order; the AUTOMATIC form
// for 6-32-32-4 up to 8192 rollouts: "row_exact" / "mfma" restore the order)
hipError_t launch_rollout_row(int hidden, int n_hidden, const RolloutArgs &a, bool tree, hipStream_t stream);
hipError_t launch_rollout_row_batch(const QuadBatchArgs &b, bool tree, hipStream_t stream);  // grid (groups, instances)

// rollout_row64.hip: latency form of 64-wide nets on the vector ALU -- r / 2 dynamics waves (two rollouts of 32 lanes each) +
// pose, cost, control and noise wave per r = 16 rollouts; hidden layers' weights from LDS, output layer as a butterfly
// (NOT the reference's summation order; never chosen automatically: config 4's vector-ALU A/B arm); a.wpack = pack_row64_weights (mppi_abi.hip)
bool row64_variant_supported(int hidden, int n_hidden);
int row64_pack_floats(int n_hidden);
hipError_t launch_rollout_row64(int hidden, int n_hidden, const RolloutArgs &a, int r, hipStream_t stream);

// rollout_m44.hip: latency form of 64-wide nets on v_mfma_f32_4x4x1 with A-matrix broadcast -- four dynamics waves (four
// rollouts each, all hidden weights in registers) + pose, cost, control and noise wave per 16 rollouts; output layer as a
// butterfly, hidden layers (split) as two accumulation chains -- NOT the reference's summation order, and the AUTOMATIC form
// for 64-wide nets up to 8192 rollouts ("m44_chain": hidden layers in the reference's order; "mfma": every layer);
// a.wpack = pack_m44_weights (mppi_abi.hip).  The group -- shared state, the dynamics wave's hand-overs with the riders, the
// group body -- is m44_group.hpp's, shared with rollout_lds44.hip and rollout_lds128.hip
bool m44_variant_supported(int hidden, int n_hidden);
int m44_pack_floats(int n_hidden);
hipError_t launch_rollout_m44(int hidden, int n_hidden, const RolloutArgs &a, bool split, hipStream_t stream);  // split: two chains per hidden layer
// the split form for the two controllers of a tick in one launch: b.n == 2, grid (groups of the larger instance, 2)
hipError_t launch_rollout_m44_batch(int n_hidden, const QuadBatchArgs &b, hipStream_t stream);

// rollout_valu.hip (generic vector-ALU kernel, any layer list)
struct NetDesc {
  int n_layers;
  int layers[8];
  int max_width;
  int num_params;
};
// a list 6 -> hidden widths 1..max_width -> 4 with at least one hidden layer: what the forms with the layer list as a kernel
// argument take (lds44, lds128, lds16)
inline bool lds_list_ok(const NetDesc &net, int max_width)
{
  if (net.n_layers < 3 || net.n_layers > 8 || net.layers[0] != kNetIn || net.layers[net.n_layers - 1] != kNetOut) return false;
  for (int l = 1; l + 1 < net.n_layers; l++)
    if (net.layers[l] < 1 || net.layers[l] > max_width) return false;
  return true;
}
size_t valu_lds_bytes(const NetDesc &net);
hipError_t launch_rollout_valu(const NetDesc &net, const RolloutArgs &a, hipStream_t stream);
// register/scalar-operand vector-ALU kernel for 6 -> H x NHID -> 4 (theta with pre-scaled hidden biases)
bool valu_reg_supported(int hidden, int n_hidden);
hipError_t launch_rollout_valu_reg(int hidden, int n_hidden, const RolloutArgs &a, hipStream_t stream);
hipError_t launch_dynamics_valu(const NetDesc &net, const float *theta, const float *states,
                                const float *controls, float *ders, int n, int negate_yaw_der,
                                hipStream_t stream);

// rollout_lds44.hip: the m44 group (m44_group.hpp: four dynamics waves x four rollouts on v_mfma_f32_4x4x1 with A-matrix broadcast + the four
// riders per 16 rollouts) for ANY layer list 6 -> hidden widths 1..64 -> 4: the layer list is a kernel argument, the weights of
// all layers are read from LDS, every layer -- the output layer too -- is one k-ascending chain (the reference's order:
// bit-identical to the other exact forms); a.wpack = pack_lds44_weights (abi_pack.hip)
constexpr int kLds44BiasQuads = 2;  // float4 per lane in front of the weights: one bias per layer
constexpr int kLds44Ahead = 3;      // float4 of weights requested ahead of their use (and zero quads behind the last layer)
bool lds44_supported(const NetDesc &net);
int lds44_pack_floats(const NetDesc &net);
hipError_t launch_rollout_lds44(const NetDesc &net, const RolloutArgs &a, hipStream_t stream);
// two instances of the SAME layer list in one launch: b.n == 2, grid (groups of the larger instance, 2)
hipError_t launch_rollout_lds44_batch(const NetDesc &net, const QuadBatchArgs &b, hipStream_t stream);

// rollout_row32.hip: the row group (row_group.hpp; rollout_row.hip's form) for ANY layer list 6 -> 1 to 4 hidden widths 1..32 -> 4: every
// hidden layer runs as a 32-wide one (neurons it does not have: weight 0, bias 0), NHH = hidden layers - 1 hidden-to-hidden chains per
// step.  Exact ("row32": the reference's order in every layer, the bits of the other exact forms; up to three hidden layers -- the
// fourth does not fit the registers) and tree ("row32_tree": row_out_tree's output layer, the bits of "row_tree" on 6-32-32-4).  A list
// of two hidden layers runs rollout_row.hip's kernels.  a.wpack = pack_row32_weights (abi_pack.hip), entries of 16 lanes x 16 B:
struct RowPackLayout {
  int w2, w3, bias, b3, tree, entries;  // first entry of: the hidden-to-hidden layers (16 each), the exact output layer (16), the
                                        // hidden biases (two layers per entry), b3, the tree's three; the image's entries
};
constexpr RowPackLayout row_pack_layout(int nhh)
{
  const int w3 = 3 + 16 * nhh, bias = w3 + 16, b3 = bias + (nhh + 2) / 2;
  return RowPackLayout{3, w3, bias, b3, b3 + 1, b3 + 4};
}
static_assert(row_pack_layout(1).bias == 35 && row_pack_layout(1).entries == 40, "NHH = 1: pack_row_weights' image");
constexpr int kRow32MaxHidden = 4, kRow32MaxHiddenExact = 3;
bool row32_supported(const NetDesc &net, bool tree);
int row32_pack_floats(const NetDesc &net);
hipError_t launch_rollout_row32(const NetDesc &net, const RolloutArgs &a, bool tree, hipStream_t stream);
// two instances of the SAME layer list in one launch: b.n == 2, grid (groups of the larger instance, 2)
hipError_t launch_rollout_row32_batch(const NetDesc &net, const QuadBatchArgs &b, bool tree, hipStream_t stream);

// rollout_lds128.hip: the lds44 group (m44_group.hpp) for ANY layer list 6 -> hidden widths 1..128 -> 4 whose image fits one workgroup's LDS:
// a hidden layer is one or two halves of 64 neurons with an accumulator each, its inputs one or two transposed activation
// sets walked k ascending (the reference's order: bit-identical to the other exact forms); a.wpack = pack_lds128_weights
constexpr int kLds128BiasQuads = 4;  // float4 per lane in front of the weights: float 2 j + h = bias of half h of weight layer j
bool lds128_supported(const NetDesc &net);
int lds128_pack_floats(const NetDesc &net);
size_t lds128_lds_bytes(const NetDesc &net);  // shared state + image of a list 6 -> 1..128 -> 4 (0 for any other list)
size_t lds128_lds_limit();                    // the dynamic LDS a group may have
hipError_t launch_rollout_lds128(const NetDesc &net, const RolloutArgs &a, hipStream_t stream);
// two instances of the SAME layer list in one launch: b.n == 2, grid (groups of the larger instance, 2)
hipError_t launch_rollout_lds128_batch(const NetDesc &net, const QuadBatchArgs &b, hipStream_t stream);

// rollout_lds16.hip: the THROUGHPUT form for ANY layer list 6 -> hidden widths 1..128 -> 4 whose image fits one workgroup's LDS:
// rollout_mfma_kernel's wave (wave16_step.hpp: 16 rollouts, the whole step, v_mfma_f32_16x16x4_f32, eps from the stand-alone generator) with the
// layer list a kernel argument and the A operands read from an LDS image, every layer in the reference's order (bit-identical
// to the other exact forms); a.wpack = pack_lds16_weights (abi_pack.hip)
struct Lds16Net {
  int n_w;      // weight layers; the last one is the output layer
  int img_f4;   // float4 of the whole image
  int mt[7];    // weight layer j: its M tiles, ceil(outputs / 16) (1 for the output layer)
  int ks[7];    // its k-steps: 2 for layer 0 (6 inputs padded to 8), else 4 x mt[j - 1]
  int off[7];   // float4 index of its A operands in the image
  int boff[7];  // float4 index of its biases
  int nout[7];  // its outputs
};
Lds16Net lds16_net_of(const NetDesc &net);    // of a list lds16_lds_bytes(net) != 0 (wave16_image.hpp builds it, for glb16 too)
bool lds16_supported(const NetDesc &net);
int lds16_pack_floats(const NetDesc &net);
size_t lds16_lds_bytes(const NetDesc &net);   // a workgroup's dynamic LDS = the image of a list 6 -> 1..128 -> 4 (0 for any other list)
size_t lds16_lds_limit();                     // the dynamic LDS a workgroup may have
// threads per workgroup for K rollouts on a device of `cus` CUs: the smallest of 256 / 512 / 1024 with every workgroup resident at once
int lds16_block_threads(const NetDesc &net, int K, int cus);
hipError_t launch_rollout_lds16(const NetDesc &net, const RolloutArgs &a, int cus, hipStream_t stream);  // cus: the device's CUs (the handle's)

// rollout_fleet16.hip: lds16's wave and image for up to kMaxFleet independent controllers of ONE layer list in one launch -- grid
// (workgroups of the largest instance, instances), the instances' argument blocks an array in device memory
constexpr int kMaxFleet = 64;
struct Fleet16Plan {
  int threads, grid_x, grid_y;  // one workgroup size for the launch; all zero: no launch (a list lds16 refuses, n outside 1..kMaxFleet)
  size_t lds_bytes;             // a workgroup's dynamic LDS: lds16_lds_bytes
};
// Ks: the instances' rollouts; threads: wave16_image_block_threads' rule on all workgroups of the fleet (n = 1: lds16_block_threads)
Fleet16Plan fleet16_plan(const NetDesc &net, const int *Ks, int n, int cus);
// h_inst: the n argument blocks on the host (K and the cost flags are read there); d_inst: the same blocks in device memory
hipError_t launch_rollout_fleet16(const NetDesc &net, const RolloutArgs *h_inst, const RolloutArgs *d_inst, int n, int cus, hipStream_t stream);

// rollout_fleet_multi.hip: the workgroup of "multi4_tree_gen" (rollout_multi.hip, nd = 44) for up to kMaxFleet independent
// controllers of ONE shape multi_variant_supported takes in one launch -- grid (64-rollout groups of the largest instance,
// instances), eight waves per workgroup, the instances' argument blocks an array in device memory
struct FleetMultiPlan {
  int threads, grid_x, grid_y;  // all zero: no launch (another shape, n outside 1..kMaxFleet, a K that is no multiple of 64)
};
FleetMultiPlan fleet_multi_plan(int hidden, int n_hidden, const int *Ks, int n);
// h_inst: the n argument blocks on the host (K is read there); d_inst: the same blocks in device memory
hipError_t launch_rollout_fleet_multi(int hidden, int n_hidden, const RolloutArgs *h_inst, const RolloutArgs *d_inst, int n, hipStream_t stream);

// rollout_glb16.hip: lds16's wave for EVERY layer list 6 -> hidden widths 1..256 -> 4 (3 <= n_layers <= 8): the image is lds16's
// with up to 16 tiles per layer; its head (biases + layer 0) and the first R blocks of its stream are resident in LDS, the other
// blocks are read from the image in global memory; a.wpack = pack_glb16_weights (abi_pack.hip).  cap: the cap on R given by
// name ("glb16_r<N>"), < 0 for none
#ifndef MPPI_GLB16_AHEAD
#define MPPI_GLB16_AHEAD 2
#endif
constexpr int kGlb16Ahead = MPPI_GLB16_AHEAD;  // blocks requested ahead of their use, and blocks of zeros behind the stream (2 or 4)
Lds16Net glb16_net_of(const NetDesc &net);     // of a list glb16_supported accepts
bool glb16_supported(const NetDesc &net);
int glb16_pack_floats(const NetDesc &net);
size_t glb16_head_bytes(const NetDesc &net);             // biases + layer 0: always resident
int glb16_stream_blocks(const NetDesc &net);             // 1 KB blocks behind the head, the zero blocks included
int glb16_resident_blocks(const NetDesc &net, int cap);  // R = min(stream blocks, floor((limit - head) / 1 KB), cap)
size_t glb16_lds_bytes(const NetDesc &net, int cap);     // a workgroup's dynamic LDS: head + R blocks
size_t glb16_lds_limit();
// threads per workgroup for K rollouts on a device of `cus` CUs: the smaller of 256 / 512 with every workgroup resident at once, else 512
int glb16_block_threads(const NetDesc &net, int K, int cus, int cap);
hipError_t launch_rollout_glb16(const NetDesc &net, const RolloutArgs &a, int cus, int cap, hipStream_t stream);
// ... and for up to kMaxFleet independent controllers, every one with its OWN layer list and cap, in one launch ("fleet_glb16") --
// grid (workgroups of the largest instance, instances); the instances' argument blocks and their layer lists are two arrays in
// device memory
struct FleetGlbNet {
  Lds16Net net;  // glb16_net_of the instance's list
  int R;         // its resident stream blocks: glb16_resident_blocks(list, cap)
};
FleetGlbNet fleet_glb16_net_of(const NetDesc &net, int cap);
struct FleetGlb16Plan {
  int tiles;                    // the instance of the launch: 16 if any list is wider than 128, else 8
  int threads, grid_x, grid_y;  // one workgroup size for the launch; all zero: no launch (a list glb16 refuses, n outside 1..kMaxFleet, a K below 16)
  size_t lds_bytes;             // a workgroup's dynamic LDS: the largest glb16_lds_bytes of the instances
};
// Ks: the instances' rollouts; threads: wave16_image_block_threads' rule on all workgroups of the fleet (n = 1: glb16_block_threads)
FleetGlb16Plan fleet_glb16_plan(const NetDesc *nets, const int *caps, const int *Ks, int n, int cus);
// h_inst: the n argument blocks on the host (K and the cost flags are read there); d_inst: the same blocks in device memory;
// d_nets: fleet_glb16_net_of(nets[i], caps[i]) of every instance in device memory
hipError_t launch_rollout_fleet_glb16(const NetDesc *nets, const int *caps, const RolloutArgs *h_inst, const RolloutArgs *d_inst, const FleetGlbNet *d_nets,
                                      int n, int cus, hipStream_t stream);

// rollout_glb44.hip: lds128's group (m44_group.hpp) for EVERY layer list 6 -> hidden widths 1..256 -> 4 (3 <= n_layers <= 8): a hidden
// layer is one to four halves of 64 neurons with an accumulator each, its inputs one to four transposed activation sets; the
// image is lds128's layout in 1 KB quads with four halves per layer; its head (bias quads + layer 0) and the first R quads of the
// stream behind it are resident in LDS, the other quads are read from the image in global memory; a.wpack = pack_glb44_weights
// (abi_pack.hip).  cap: the cap on R given by name ("glb44_r<N>"), < 0 for none
#ifndef MPPI_GLB44_AHEAD
#define MPPI_GLB44_AHEAD 8
#endif
#ifndef MPPI_GLB44_AHEAD_LDS
#define MPPI_GLB44_AHEAD_LDS 3
#endif
constexpr int kGlb44Ahead = MPPI_GLB44_AHEAD;         // streamed quads requested ahead of their use, and quads of zeros behind the stream
constexpr int kGlb44AheadLds = MPPI_GLB44_AHEAD_LDS;  // resident quads requested ahead of their use (kLds44Ahead)
constexpr int kGlb44BiasQuads = 7;             // float4 per lane in front of the weights: quad j, float h = bias of half h of weight layer j
bool glb44_supported(const NetDesc &net);
int glb44_pack_floats(const NetDesc &net);
size_t glb44_head_bytes(const NetDesc &net);             // bias quads + layer 0: always resident
int glb44_stream_quads(const NetDesc &net);              // 1 KB quads behind the head, the zero quads included
int glb44_resident_quads(const NetDesc &net, int cap);   // R = min(stream quads, floor((limit - shared state - head) / 1 KB), cap)
size_t glb44_lds_bytes(const NetDesc &net, int cap);     // a group's dynamic LDS: shared state + head + R quads
size_t glb44_lds_limit();
hipError_t launch_rollout_glb44(const NetDesc &net, const RolloutArgs &a, int cap, hipStream_t stream);
// two instances of the SAME layer list and cap in one launch: b.n == 2, grid (groups of the larger instance, 2)
hipError_t launch_rollout_glb44_batch(const NetDesc &net, const QuadBatchArgs &b, int cap, hipStream_t stream);

// rollout_bf.hip (GeneralizedLinear basis-function dynamics, W[4][25] in a.wpack)
hipError_t launch_rollout_bf(const RolloutArgs &a, int waves, hipStream_t stream);  // waves per 64 rollouts: 1, 2, 3
// several instances of the three-wave form in one launch (grid: groups of 64 rollouts x instances)
hipError_t launch_rollout_bf_batch(const QuadBatchArgs &b, hipStream_t stream);
hipError_t launch_dynamics_bf(const float *W, const float *states, const float *controls, float *ders, int n,
                              hipStream_t stream);

// rollout_fleet_bf.hip: the workgroups of rollout_bf.hip (bf_group.hpp) for up to kMaxFleet independent controllers of the
// basis-function model in one launch -- grid (64-rollout groups of the largest instance, instances), one wave count for the
// launch, the instances' argument blocks an array in device memory, eps from every instance's noise buffer
struct FleetBfPlan {
  int waves, threads, grid_x, grid_y;  // all zero: no launch (n outside 1..kMaxFleet, a K that is no multiple of 64, forced_waves outside 0..3)
};
// Ks: the instances' rollouts; simds: the device's SIMDs; forced_waves: 1..3, or 0 for form_of's rule on the groups of the whole
// fleet G = sum K / 64 (3 waves while 3 G <= simds, 2 while G <= simds, else 1; n = 1: form_of's choice for that handle)
FleetBfPlan fleet_bf_plan(const int *Ks, int n, int simds, int forced_waves);
// h_inst: the n argument blocks on the host (K is read there); d_inst: the same blocks in device memory
hipError_t launch_rollout_fleet_bf(const RolloutArgs *h_inst, const RolloutArgs *d_inst, int n, int simds, int forced_waves, hipStream_t stream);

// rollout_bf_row.hip: latency form of the basis-function model -- four dynamics waves (four rollouts each, a rollout's sixteen
// (output, y-thread) cells on one DPP row) + pose, cost, control and noise wave per 16 rollouts; a.wpack = the per-lane image
// (pack_bf_row_weights, abi_pack.hip): 16-B entry e of lane p = 4 j + y at float4 index e * 16 + p; slot m of a lane is basis
// function i = y + 4 m.  Entries 0, 1: the weights W[j][y + 4 m] (0 where i > 24) and, in the last word, the lane's marks;
// 2, 3: the divisors c (1 for a plain basis function); 4, 5: RN(1 / c) in fp32
constexpr int kBfRowSlots = 7, kBfRowPackEntries = 6;
// marks, one bit per slot m each, shifted left by m: the basis function is its numerator (no quotient); it is 0 unless
// u_x >= 0.1 (BasisShared::big); the slot exists (i <= 24).  kBfRowDouble: slot 3 is a double quotient (i = 13, 14)
constexpr unsigned kBfRowPlain = 1u, kBfRowBigOnly = 1u << 8, kBfRowUsed = 1u << 16, kBfRowDouble = 1u << 24;
int bf_row_pack_floats();
hipError_t launch_rollout_bf_row(const RolloutArgs &a, hipStream_t stream);
hipError_t launch_rollout_bf_row_batch(const QuadBatchArgs &b, hipStream_t stream);  // two instances: grid (groups, 2)

// rollout_trace.hip: chosen rollouts of a finished solve replayed with their records (mppi_trace_rollouts) -- one wavefront per
// rollout and one lane per neuron for ANY layer list (every neuron the reference's chain: costs bit-identical to the exact
// forms), one lane per rollout for the basis-function model
struct TraceArgs {
  float state[kStateDim];
  const float *V;       // [T][K][2] the solve's applied controls, before the clamp
  const int *ks;        // [n] rollout indices, each in [0, K)
  const float *wimg;    // network: pack_trace_weights (abi_pack.hip); basis functions: W[4][25]
  const double *inv_t;  // as RolloutArgs::inv_t
  // outputs, slot i = rollout ks[i]; any may be nullptr
  float *states;        // [n][T][7] the state before the update of step t
  float *controls;      // [n][T][2] after the clamp
  float *step_costs;    // [n][T]    computeCost of step t (0 at t = 0)
  float *costs;         // [n]       the running mean
  int *first_crash;     // [n]       the first step whose cost saw the crash flag, -1: never
  int n, K, T;
  float nu[2], u_lo[2], u_hi[2], dt;
  int negate_yaw_der;
  CostArgs cost;
};
bool trace_image_in_lds(const NetDesc &net);  // the k-major image and the waves' tiles fit the kernel's LDS budget
hipError_t launch_rollout_trace(const NetDesc &net, const TraceArgs &a, hipStream_t stream);
hipError_t launch_rollout_trace_bf(const TraceArgs &a, hipStream_t stream);
// ... and the traces of n <= kMaxFleet independent controllers in one launch (mppi_trace_rollouts_batch): grid (workgroups of the
// member with the most rollouts, members), the members' argument blocks an array in device memory.  Members may differ in
// everything a TraceArgs holds and in their layer lists; rollout_trace_fleet_kernel serves the network model,
// rollout_trace_fleet_bf_kernel the basis-function model (net and img_lds unused)
struct TraceFleetArgs {
  TraceArgs a;   // a.n: the member's rollouts (0: none); a.ks: its piece of the device index array
  int img_lds;   // the image is copied to LDS (trace_image_in_lds)
  NetDesc net;
};
hipError_t launch_rollout_trace_fleet(const TraceFleetArgs *h_inst, const TraceFleetArgs *d_inst, int n, hipStream_t stream);
hipError_t launch_rollout_trace_fleet_bf(const TraceFleetArgs *h_inst, const TraceFleetArgs *d_inst, int n, hipStream_t stream);
// trace_select_fleet_kernel, in front of the two on the same stream: ks[r] (and ks_out[r] where given) = the rollout of rank r < n
// in mppi_top_rollouts' order -- a number before a NaN, the larger weight first, the lower index first -- chosen from the
// member's K device weights.  w == nullptr or n == 0: a member that brought its indices, nothing is written
struct TraceSelectArgs {
  const float *w;  // [K] the solve's weights (d_w)
  int *ks;         // [n] the member's piece of the device index array
  int *ks_out;     // [n] a copy in the result buffer, or nullptr
  int K, n;
};
hipError_t launch_trace_select_fleet(const TraceSelectArgs *h_inst, const TraceSelectArgs *d_inst, int n, hipStream_t stream);

// solve_kernels.hip
// everything of one solve iteration after the rollout (solve_tail_kernel up to 4096 rollouts, solve_tail_stream_kernel beyond)
struct TailLaunch {
  const float *costs, *V, *hist;
  float *U, *w, *scal, *res, *slid;
  unsigned *counter;
  int K, T, last_iter, slide_stride;
  unsigned seq;
  float gamma, init0, init1;
  // K > 4096 (solve_tail_stream_kernel): granule buffers (gx: 3 x 64 exchange granules; gpart: [T][K/64][2] chain results,
  // 8 B each, zero when allocated), the tag of this launch's granules (never 0, never the tag of an earlier launch on these
  // buffers), the deadline of every in-launch wait in 100 MHz ticks, and the tests' fault role (0: none)
  unsigned long long *ug = nullptr;  // [T][2] granules of the raw weighted mean (every form)
  int no_device_copy = 0;            // chained ticks: publish only
  float *hist_out = nullptr;         // chained ticks, last solve: where the smoothing workgroup leaves hist[4]
  unsigned long long *gx = nullptr, *gpart = nullptr;
  unsigned epoch = 0, poll_ticks = 0;
  int fault = 0;
  // the rollout launch's minimum cost (mppi_device.hpp: publish_min_cost) and that launch's tag; nullptr: the tail reduces the costs itself
  const unsigned long long *min_cost = nullptr;
  unsigned min_cost_tag = 0;
};
// does a solve of K rollouts run the one-launch streaming tail (in-launch column exchanges; wait_pending then also checks the
// published rows for the NaN a timed-out wait leaves)?
bool tail_is_stream(int K);
constexpr int kTailExchangeGranules = 3 * 64 + 32 * 16 + 32 * 64;  // solve_kernels.hip: 3 x kMaxChunks + kBcastReplicas lines + kBcastReplicas x kMaxChunks
hipError_t launch_solve_tail(const TailLaunch &l, hipStream_t stream);
// the tails of n <= kMaxBatch instances (K <= 4096 each) in one launch
hipError_t launch_solve_tail_batch(const TailLaunch *l, int n, hipStream_t stream);
// the tails of n <= kMaxFleet instances (K <= 4096 each) in one launch, their argument blocks an array in device memory
// (solve_tail_fleet_kernel): fill_solve_tail_fleet writes the n blocks, solve_tail_fleet_arg_bytes() each, where the host
// stages them; d_args: the same blocks in device memory, complete once `stream` reaches the launch
size_t solve_tail_fleet_arg_bytes();
void fill_solve_tail_fleet(void *dst, const TailLaunch *l, int n);
hipError_t launch_solve_tail_fleet(const TailLaunch *l, int n, const void *d_args, hipStream_t stream);
hipError_t launch_debug_cost(const CostArgs &c, float x, float y, float heading, int width_m, int height_m,
                             int ppm, float *out, hipStream_t stream);
hipError_t launch_slide(float *in, int T, int stride, float init0, float init1, hipStream_t stream);
hipError_t launch_kt_to_tk(const float *src, float *dst, int K, int T, hipStream_t stream);
hipError_t launch_tk_to_kt(const float *src, float *dst, int K, int T, hipStream_t stream);

// noise_mrg32k3a.hip
hipError_t launch_noise(const uint32_t *rng_in, uint32_t *rng_out, const uint32_t *jump, int K, int T,
                        int L, int C, float *eps, hipStream_t stream);
// the draws of n <= kMaxFleet instances in one launch (noise_fleet_kernel): noise_kernel over an array of descriptors in device
// memory, grid (blocks of the largest instance, instances).  K == 0: an instance that draws nothing (explicit noise)
struct NoiseFleetDesc {
  const uint32_t *rng_in;
  uint32_t *rng_out;
  const uint32_t *jump;
  float *eps;
  int K, T, L, C;
};
hipError_t launch_noise_fleet(const NoiseFleetDesc *h_desc, const NoiseFleetDesc *d_desc, int n, hipStream_t stream);
hipError_t launch_noise_init(uint32_t *rng, int K, const uint32_t base[6], const uint32_t *sub,
                             int sub_bits, const uint32_t *one, uint64_t offset, hipStream_t stream);

// ddp_fleet.hip: the DDP feedback gains (ddp_feedback.cpp's pass for the network model) of n <= kMaxFleet independent controllers
// in one launch, one workgroup per controller, the instances' argument blocks an array in device memory.
//   in:   [7] x0 | [T][7] target_x | [T][2] target_u
//   out:  DdpResult's arrays -- [T][2][7] feedback | [T][2] feedforward | [T][7] x | [T][2] u | [T] cost -- then total_cost and one
//         status word (0: done; 1: a 2 x 2 control Hessian could not be factorised, the arrays are void)
//   work: [T][7] x and [T][2] u of the initial rollout | [T][2] sin, cos of its headings | [T][72] df and dL | [T][hidden] tanh values
struct DdpFleetArgs {
  const float *theta;  // the weights as the reference packs them (row-major; the Jacobians)
  const float *wimg;   // pack_trace_weights: every W transposed (the forward passes)
  const float *in;
  float *out, *work;
  int T, negate_yaw_der;
  int img_lds;         // the image is copied to LDS (ddp_fleet_image_in_lds)
  float dt;
  float u_lo[2], u_hi[2], Q[7], R[2], Qf[7];
  NetDesc net;
};
__host__ __device__ inline int ddp_fleet_hidden(const NetDesc &net)
{
  int s = 0;
  for (int l = 1; l + 1 < net.n_layers; l++) s += net.layers[l];
  return s;
}
inline size_t ddp_fleet_in_floats(int T) { return 7 + (size_t)9 * T; }
inline size_t ddp_fleet_out_floats(int T) { return (size_t)26 * T + 2; }
inline size_t ddp_fleet_work_floats(int T, const NetDesc &net) { return (size_t)T * (7 + 2 + 2 + 72 + ddp_fleet_hidden(net)); }
bool ddp_fleet_image_in_lds(const NetDesc &net);
hipError_t launch_ddp_fleet(const DdpFleetArgs *h_inst, const DdpFleetArgs *d_inst, int n, hipStream_t stream);
// out[i] = tanhf_scalar(in[i]) on the device (mppi_debug_device_tanhf)
hipError_t launch_device_tanhf(const float *in, float *out, size_t n, hipStream_t stream);

// nominal_fleet.hip: the nominal trajectories (mppi_nominal_traj's replay for the network model) of n <= kMaxFleet independent
// controllers in one launch, one workgroup per controller, the instances' argument blocks an array in device memory.
//   in:   [7] state | [T][2] the control sequence (before the clamp)
//   out:  [T][7] state_seq | [T][2] control_seq (clamped)
struct NominalFleetArgs {
  const float *wimg;   // pack_trace_weights: every W transposed
  const float *in;
  float *out;
  int T, negate_yaw_der;
  int img_lds;         // the image is copied to LDS (nominal_fleet_image_in_lds)
  float dt;
  float u_lo[2], u_hi[2];
  NetDesc net;
};
inline size_t nominal_fleet_in_floats(int T) { return 7 + (size_t)2 * T; }
inline size_t nominal_fleet_out_floats(int T) { return (size_t)9 * T; }
bool nominal_fleet_image_in_lds(const NetDesc &net);
hipError_t launch_nominal_fleet(const NominalFleetArgs *h_inst, const NominalFleetArgs *d_inst, int n, hipStream_t stream);

// plant_fleet.hip: the plant step of a fleet's closed loop on the device (mppi_closed_loop_ticks_batch) -- the first `stride` steps of
// nominal_fleet_kernel's replay (its text, its bits) from the controller's device state slot with the controls the tail kernel of
// tick `tick` smoothed, one workgroup per controller, the argument blocks an array in device memory that is sent ONCE per run: what
// changes from tick to tick is the launch's `tick` (which of the two [U | hist] buffers, which log rows).
struct PlantFleetArgs {
  const float *wimg;    // pack_trace_weights: every W transposed
  const float *U_even;  // [T][2] the smoothed sequence of the run's even ticks (not yet slid) ...
  const float *U_odd;   // ... and of its odd ticks (the other buffer where the tail's slid copy is swapped in, else the same one)
  const float *scal;    // the tail's scalars: [1] eta, [2] the trajectory cost
  float *state;         // [7] the controller's device state slot: in, and out
  float *log_x;         // [ticks + 1][7]: row tick + 1 receives the new state (row 0 is the host's)
  float *log_u;         // [ticks][stride][2]: the clamped controls the plant applied
  float *log_c;         // [ticks]: the trajectory cost
  float *log_e;         // [ticks]: eta
  int T, negate_yaw_der, stride;
  float dt;
  float u_lo[2], u_hi[2];
  NetDesc net;
};
// d_ra: the fleet's rollout argument blocks in device memory -- instance i's RolloutArgs::state (a by-value field at offset 0) receives
// the new state too -- or nullptr (behind the run's last tick)
hipError_t launch_plant_fleet(const PlantFleetArgs *h_inst, const PlantFleetArgs *d_inst, RolloutArgs *d_ra, int n, int tick, hipStream_t stream);

// plant_drive_fleet.hip: a plant of its own for a fleet (mppi_plant_drive_batch, mppi_closed_loop_sim_batch) -- `periods` control
// periods of `substeps` plant steps each on the PLANT's network (mppi_set_plant_model; else the handle's own), driven by the law of
// include/mppi_hip.h: the nominal controls interpolated between rows lo and lo + 1 in double, optionally the DDP feedback
// K (x - x_des) in fp32, the handle's clamp, one step of nom_step's text with dt / substeps.  One wave per controller, the argument
// blocks an array in device memory.  The closed loop sends them ONCE per run and passes the tick with the launch, as
// plant_fleet_kernel's; the batched call launches with tick 0.
constexpr int kPlantDriveMaxSubsteps = 16;
struct PlantDriveArgs {
  const float *wimg;       // pack_trace_weights of the plant's network
  const float *useq_even;  // [periods + 1 ..][2] the nominal controls: control_seq rows, or (clamp_rows) the smoothed U of the run's even ticks ...
  const float *useq_odd;   // ... and of its odd ticks (the batched call: the same pointer)
  const float *xseq;       // [periods + 1 ..][7] the nominal states; nullptr without feedback
  const float *gains;      // [periods + 1 ..][2][7] the feedback gains; nullptr without feedback
  const float *state_in;   // [7] the start state ...
  float *state_out;        // ... and where the new one goes (the closed loop: the same slot)
  float *applied;          // [ticks][periods * substeps][2] the applied controls, or nullptr
  const float *scal;       // closed loop: the tail's scalars ([1] eta, [2] the trajectory cost); nullptr: no log_c / log_e
  float *log_x;            // closed loop: [ticks + 1][7], row tick + 1 receives the new state; or nullptr
  float *log_c, *log_e;    // closed loop: [ticks] the trajectory cost and eta
  int periods, substeps, negate_yaw_der;
  int feedback;            // apply K (x - x_des)
  int clamp_rows;          // the rows of useq are the raw U: clamp each before it is used (the closed loop without a replay launch)
  int img_lds;             // the image is copied to LDS (plant_drive_image_in_lds)
  float dt_sub;            // dt / (float)substeps
  float u_lo[2], u_hi[2];
  double a[kPlantDriveMaxSubsteps];  // a[j] = (double)j / (double)substeps
  NetDesc net;             // the plant's layer list
};
bool plant_drive_image_in_lds(const NetDesc &net);
// d_ra: as launch_plant_fleet's -- instance i's RolloutArgs::state receives the new state too -- or nullptr
hipError_t launch_plant_drive_fleet(const PlantDriveArgs *h_inst, const PlantDriveArgs *d_inst, RolloutArgs *d_ra, int n, int tick, hipStream_t stream);

// nominal_gains_fleet.hip: the nominal replay AND the DDP pass that tracks it (mppi_nominal_and_gains_batch) of n <= kMaxFleet
// independent controllers in one launch, one workgroup per controller: the replay runs on wave 1 while wave 0 runs the pass's
// initial rollout; the targets never leave the device.
//   in:   [7] state | [T][2] the control sequence (before the clamp)
//   out:  DdpFleetArgs's out (26 T + 2 floats, rounded up to four) | [T][7] state_seq | [T][2] control_seq (clamped): the pass's targets
//   work: DdpFleetArgs's work
struct NominalGainsFleetArgs {
  const float *theta;  // the weights as the reference packs them (row-major; the Jacobians)
  const float *wimg;   // pack_trace_weights: every W transposed (the forward passes of both waves)
  const float *in;
  float *out, *work;
  int T, negate_yaw_der;
  int img_lds;         // the image is copied to LDS (nominal_gains_fleet_image_in_lds)
  float dt;            // the pass's: (float)(1 / hz)
  float dt_nominal;    // the replay's: the handle's dt
  float u_lo[2], u_hi[2], Q[7], R[2], Qf[7];
  NetDesc net;
};
inline size_t nominal_gains_fleet_seq_offset(int T) { return (ddp_fleet_out_floats(T) + 3) & ~(size_t)3; }
inline size_t nominal_gains_fleet_out_floats(int T) { return nominal_gains_fleet_seq_offset(T) + nominal_fleet_out_floats(T); }
bool nominal_gains_fleet_image_in_lds(const NetDesc &net);
hipError_t launch_nominal_gains_fleet(const NominalGainsFleetArgs *h_inst, const NominalGainsFleetArgs *d_inst, int n, hipStream_t stream);

}  // namespace mppi
