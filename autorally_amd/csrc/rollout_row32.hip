// rollout_row32.hip -- the row group (row_group.hpp: rollout_row.hip's latency form, the network on the vector ALU with every
// weight in registers) for ANY layer list 6 -> one to four hidden layers of width 1..32 -> 4, by name only:
//   "row32"       the reference's k-ascending order in every layer: the bits of "valu_lds", "lds44" and the oracle's mode 1 (on
//                 6-32-32-4: of "row_exact"); one to three hidden layers;
//   "row32_tree"  the output layer as row_out_tree's butterfly: the oracle's mode 2 (on 6-32-32-4: the bits of "row_tree"); one to
//                 four hidden layers.
// A layer narrower than 32 runs as a 32-wide one whose missing neurons have weight 0 and bias 0 (row_group.hpp says what that can
// change: the sign of a zero).  NHH = hidden layers - 1 in {0, 2, 3} are this file's kernels; a list of two hidden layers (NHH = 1)
// runs rollout_row.hip's on the same image, whose NHH = 1 layout is pack_row_weights'.
//
// The exact form of four hidden layers is not built: (3 x 32 + 32 + 6) weight pairs of two registers are 268 registers before anything else, and a
// 512-thread group has 256 per lane -- the compiler spills 61 registers to 200-600 B of scratch inside the T loop.
//
// Of the four (AFFINE, CTRL) instances of a kernel two are built, the fast one (affine map transform, no control cost) and the
// general one, an exact superset (rollout_mfma.hip; launch_rollout_row_batch picks the same way for a mixed batch): 5 (NHH, tree)
// x 4 (single, gated, pair, gated pair) x 2 = 40 kernels.  The pair is QuadBatchArgsT<2>; three or four handles solve one by one.
//
// Registers (every kernel: 0 bytes of scratch, profiles/): from NHH = 2 a group is alone on its CU, so K beyond 16 x CUs runs in
// rounds -- correct, and not what the form is for.  LDS: the group's RowShared, as rollout_row.hip.
#include "row_group.hpp"

namespace mppi {

template <int NHH, bool AFFINE, bool CTRL, bool TREE, bool GATED>
__global__ __launch_bounds__(512) void rollout_row32_kernel(const RolloutArgs a)
{
  __shared__ __attribute__((aligned(16))) RowShared<32> sh;
  row_group<32, NHH, AFFINE, CTRL, TREE, GATED>(a, sh);
}

// two instances in one launch: grid (groups of the larger instance, 2), workgroup (x, y) runs group x of instance y
// (MPPI_BATCH_DISPATCH, mppi_device.hpp); gated: every instance's block carries its own handle's gate block
template <int NHH, bool AFFINE, bool CTRL, bool TREE, bool GATED>
__global__ __launch_bounds__(512) void rollout_row32_batch_kernel(const QuadBatchArgsT<2> b)
{
  __shared__ __attribute__((aligned(16))) RowShared<32> sh;
#define MPPI_ROW32_BODY(A)                                                                                 \
  do {                                                                                                     \
    if ((int)blockIdx.x >= (A).K / kRolloutsPerWave) return; /* the smaller instance of the two */         \
    row_group<32, NHH, AFFINE, CTRL, TREE, GATED>((A), sh);                                                \
  } while (0)
  MPPI_BATCH_DISPATCH(2, b, MPPI_ROW32_BODY);
#undef MPPI_ROW32_BODY
}

// every list 6 -> one to four (exact: three) hidden widths 1..32 -> 4
bool row32_supported(const NetDesc &net, bool tree)
{
  return lds_list_ok(net, 32) && net.n_layers - 2 <= (tree ? kRow32MaxHidden : kRow32MaxHiddenExact);
}

int row32_pack_floats(const NetDesc &net)
{
  return row32_supported(net, true) ? row_pack_layout(net.n_layers - 3).entries * 16 * 4 : 0;
}

namespace {
// f(integral_constant NHH, TREE, fast, GATED) for the instance a list needs; false: no such kernel
template <class F>
hipError_t row32_dispatch(int nhh, bool tree, bool fast, bool gated, F f)
{
  auto flags = [&](auto n, auto tr) {
    if (fast) return gated ? f(n, tr, std::true_type{}, std::true_type{}) : f(n, tr, std::true_type{}, std::false_type{});
    return gated ? f(n, tr, std::false_type{}, std::true_type{}) : f(n, tr, std::false_type{}, std::false_type{});
  };
  if (tree) {
    if (nhh == 0) return flags(std::integral_constant<int, 0>{}, std::true_type{});
    if (nhh == 2) return flags(std::integral_constant<int, 2>{}, std::true_type{});
    if (nhh == 3) return flags(std::integral_constant<int, 3>{}, std::true_type{});
  } else {
    if (nhh == 0) return flags(std::integral_constant<int, 0>{}, std::false_type{});
    if (nhh == 2) return flags(std::integral_constant<int, 2>{}, std::false_type{});
  }
  return hipErrorInvalidValue;
}
}  // namespace

hipError_t launch_rollout_row32(const NetDesc &net, const RolloutArgs &a, bool tree, hipStream_t stream)
{
  if (!row32_supported(net, tree) || a.K % kRolloutsPerWave != 0) return hipErrorInvalidValue;
  const int nhh = net.n_layers - 3;
  if (nhh == 1) return launch_rollout_row(32, 2, a, tree, stream);  // the image's NHH = 1 layout is that kernel's
  const bool fast = a.cost.affine != 0 && a.cost.need_control_cost == 0;
  const dim3 grid(a.K / kRolloutsPerWave), block(512);
  return row32_dispatch(nhh, tree, fast, a.gate != nullptr, [&](auto n, auto tr, auto fa, auto ga) {
    constexpr bool kFast = decltype(fa)::value;
    MPPI_LAUNCH_ROLLOUT((rollout_row32_kernel<decltype(n)::value, kFast, !kFast, decltype(tr)::value, decltype(ga)::value>), grid, block, 0, stream, a);
    return hipGetLastError();
  });
}

hipError_t launch_rollout_row32_batch(const NetDesc &net, const QuadBatchArgs &b, bool tree, hipStream_t stream)
{
  BatchFlags f;
  if (b.n != 2 || !row32_supported(net, tree) || !batch_flags_of(b, f)) return hipErrorInvalidValue;
  const int nhh = net.n_layers - 3;
  if (nhh == 1) return launch_rollout_row_batch(b, tree, stream);
  const QuadBatchArgsT<2> b2 = batch_args_prefix<2>(b);
  const dim3 grid(f.gmax, 2), block(512);
  return row32_dispatch(nhh, tree, f.affine && !f.ctrl, f.gated, [&](auto n, auto tr, auto fa, auto ga) {
    constexpr bool kFast = decltype(fa)::value;
    hipLaunchKernelGGL((rollout_row32_batch_kernel<decltype(n)::value, kFast, !kFast, decltype(tr)::value, decltype(ga)::value>), grid, block, 0, stream, b2);
    return hipGetLastError();
  });
}

}  // namespace mppi
