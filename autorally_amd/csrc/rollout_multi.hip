// rollout_multi.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) for gfx950, the form for K beyond
// the latency regime: ND "dynamics" wavefronts (16 rollouts each, the whole network on the matrix
// instruction, mfma_net.hpp) + ONE cost wavefront (two at ND = 4: pose | cost) + ONE control wavefront per
// workgroup of 16 ND rollouts.  The workgroup itself -- what every wave does and why -- is multi_group.hpp's
// multi_group; the kernel here runs group blockIdx.x of its kernel argument.
#include "multi_group.hpp"

namespace mppi {

// SPLIT_: the pose and fetch riders of the ND = 4 form (eight waves per workgroup); ND = 2 runs one cost wave.
// GATED (the automatic ND = 4 tree form only): enqueued one solve ahead (a.gate != nullptr)
template <int H, int NHID, int ND, bool SPLIT_ = (ND == 4), bool TREE = false, bool GATED = false>
__global__ __launch_bounds__((ND + 2 + (SPLIT_ ? 2 : 0)) * 64, (ND == 4 && !SPLIT_) ? 3 : 1) void rollout_multi_kernel(const RolloutArgs a)
{
  multi_group<H, NHID, ND, SPLIT_, TREE, GATED>(a, (int)blockIdx.x);
}

template <int H, int NHID>
static hipError_t launch_multi_t(const RolloutArgs &a, int nd, hipStream_t stream)
{
  if (a.gate != nullptr) {  // gated: the automatic form only (abi_solve.hip: chain_ok)
    if (nd != 44) return hipErrorInvalidValue;
    MPPI_LAUNCH_ROLLOUT((rollout_multi_kernel<H, NHID, 4, true, true, true>), dim3(a.K / 64), dim3(8 * 64), 0, stream, a);
    return hipGetLastError();
  }
  if (nd == 44) MPPI_LAUNCH_ROLLOUT((rollout_multi_kernel<H, NHID, 4, true, true>), dim3(a.K / 64), dim3(8 * 64), 0, stream, a);  // tree output layer
  else if (nd == 4) MPPI_LAUNCH_ROLLOUT((rollout_multi_kernel<H, NHID, 4>), dim3(a.K / 64), dim3(8 * 64), 0, stream, a);
  else if (nd == 2) MPPI_LAUNCH_ROLLOUT((rollout_multi_kernel<H, NHID, 2>), dim3(a.K / 32), dim3(4 * 64), 0, stream, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// 6-64-64-64-64-4 is left to the other forms: its 284 weight registers per lane do not fit a wave of a
// six-wave workgroup (256 VGPRs) without spilling
bool multi_variant_supported(int hidden, int n_hidden)
{
  return (hidden == 32 && (n_hidden == 2 || n_hidden == 4)) || (hidden == 64 && n_hidden == 2);
}

hipError_t launch_rollout_multi(int hidden, int n_hidden, const RolloutArgs &a, int nd, hipStream_t stream)
{
  if (nd != 2 && nd != 4 && nd != 44) return hipErrorInvalidValue;  // 44: ND = 4 with the tree output layer
  if (a.K % (16 * (nd == 44 ? 4 : nd)) != 0) return hipErrorInvalidValue;
  if (hidden == 32 && n_hidden == 2) return launch_multi_t<32, 2>(a, nd, stream);
  if (hidden == 64 && n_hidden == 2) return launch_multi_t<64, 2>(a, nd, stream);
  if (hidden == 32 && n_hidden == 4) return launch_multi_t<32, 4>(a, nd, stream);
  return hipErrorInvalidValue;
}

}  // namespace mppi

#ifdef MPPI_STAMPS
extern "C" int mppi_debug_read_multi_stamps(unsigned long long *out)
{
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mppi::g_multi_stamps), sizeof(unsigned long long) * 8);
}
#endif
