// rollout_fleet16.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) for gfx950, the lds16 wave (rollout_lds16.hip: one wavefront =
// 16 rollouts on v_mfma_f32_16x16x4_f32, the A operands from an LDS image, the reference's order: bit-identical to "valu_lds")
// for a FLEET of up to kMaxFleet independent controllers of one layer list in ONE launch.  Grid (workgroups of the largest
// instance, instances); workgroup (x, y) runs workgroup x of inst[y], where inst is an array of argument blocks in DEVICE
// MEMORY (64 blocks do not fit the kernel-argument segment): the index is workgroup-uniform and the array read-only behind a
// __restrict__ pointer, so the block arrives in scalar registers exactly as a kernel argument does (profiles/r21_a_fleet16_isa.txt:
// s_load from the instance's address, 0 bytes of scratch -- the pitfall of a run-time-indexed COPY of a block in the argument
// segment is recorded at MPPI_BATCH_DISPATCH, mppi_device.hpp).  A workgroup that holds no wave of its instance leaves before it
// stages anything and before the barrier.  Every instance stages its OWN image (the instances share the layer list, not the
// weights).  The step itself is wave16_rollout over Wave16ImageNet<MTM, Lds16Stream>, unchanged.
#include "wave16_image.hpp"
#include "wave16_step.hpp"

namespace mppi {

static int fleet16_tiles_max(const NetDesc &net) { return wave16_image_tiles_max(net, 4); }  // lds16's two instances: 4 tiles or 8

// The plan of a launch: wave16_image_block_threads' rule on the waves of the whole fleet (ONE workgroup size serves the launch;
// for n = 1 it is lds16_block_threads), grid x = the workgroups of the largest instance, grid y = the instances, the dynamic
// LDS = the image.  All zero for a list the form does not take, n outside 1..kMaxFleet or a K below one wave.
Fleet16Plan fleet16_plan(const NetDesc &net, const int *Ks, int n, int cus)
{
  Fleet16Plan p{};
  if (!lds16_supported(net) || !Ks || n < 1 || n > kMaxFleet || cus < 1) return p;
  int kmax = 0;
  for (int i = 0; i < n; i++) {
    if (Ks[i] < kRolloutsPerWave) return p;
    kmax = Ks[i] > kmax ? Ks[i] : kmax;
  }
  const bool wide = fleet16_tiles_max(net) == 8;
  p.lds_bytes = lds16_lds_bytes(net);
  p.threads = wave16_image_block_threads(Ks, n, cus, p.lds_bytes, kLds16MaxBytes, wide ? kLds16WavesPerSimd8 : kLds16WavesPerSimd4,
                                         wide ? kLds16MaxThreads8 : 1024);
  const int wpb = p.threads / 64;
  p.grid_x = (kmax / kRolloutsPerWave + wpb - 1) / wpb;
  p.grid_y = n;
  return p;
}

extern __shared__ __attribute__((aligned(16))) unsigned char fleet16_smem[];

template <int MTM, bool AFFINE, bool CTRL, int THREADS>
__global__ __launch_bounds__(THREADS) void rollout_fleet16_kernel(const RolloutArgs *__restrict__ inst, const int n, const Lds16Net net)
{
  if ((int)blockIdx.y >= n) return;
  RolloutArgs a = inst[blockIdx.y];  // workgroup-uniform, read-only: scalar loads
  // the pointers it holds are global memory, as those of a kernel argument are known to be
  a.U = load_global_ptr(inst[blockIdx.y].U);
  a.noise = load_global_ptr(inst[blockIdx.y].noise);
  a.costs = load_global_ptr(inst[blockIdx.y].costs);
  a.wpack = load_global_ptr(inst[blockIdx.y].wpack);
  a.inv_t = load_global_ptr(inst[blockIdx.y].inv_t);
  a.cost.map = load_global_ptr(inst[blockIdx.y].cost.map);
  // no wave of this workgroup belongs to the instance (a smaller K than the largest): nothing staged, no barrier
  if ((int)(blockIdx.x * (blockDim.x >> 6)) * kRolloutsPerWave >= a.K) return;
  f32x4 *const img = reinterpret_cast<f32x4 *>(fleet16_smem);
  const f32x4 *const src = reinterpret_cast<const f32x4 *>(a.wpack);
  for (int q = threadIdx.x; q < net.img_f4; q += blockDim.x) img[q] = src[q];  // the image is in LDS order, 16 B per thread and pass
  __syncthreads();  // the only barrier
  Wave16ImageNet<MTM, Lds16Stream> nn(img, src, net, 0);
  wave16_rollout<AFFINE, CTRL>(a, nn);  // the step: wave16_step.hpp (its absent waves of the last workgroup leave there)
}

template <auto KERN>
static hipError_t fleet16_launch(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const RolloutArgs *d_inst, int n, const Lds16Net &nd)
{
  if (hipError_t e = raise_lds_limit_once<KERN>(kLds16MaxBytes); e != hipSuccess) return e;
  MPPI_LAUNCH_ROLLOUT(KERN, grid, block, lds, stream, d_inst, n, nd);
  return hipGetLastError();
}

// h_inst: the host's copy of the n argument blocks (the plan and the instance are read from it); d_inst: the same blocks in
// device memory, complete once `stream` reaches the launch.  Every instance: one layer list, one pair (affine, control cost).
hipError_t launch_rollout_fleet16(const NetDesc &net, const RolloutArgs *h_inst, const RolloutArgs *d_inst, int n, int cus, hipStream_t stream)
{
  if (!h_inst || !d_inst || n < 1 || n > kMaxFleet) return hipErrorInvalidValue;
  int Ks[kMaxFleet];
  for (int i = 0; i < n; i++) {
    const RolloutArgs &a = h_inst[i];
    if (a.K % 64 != 0 || a.gate != nullptr || a.cost.affine != h_inst[0].cost.affine || a.cost.need_control_cost != h_inst[0].cost.need_control_cost)
      return hipErrorInvalidValue;
    Ks[i] = a.K;
  }
  const Fleet16Plan p = fleet16_plan(net, Ks, n, cus);
  if (p.threads == 0) return hipErrorInvalidValue;
  const dim3 grid(p.grid_x, p.grid_y), block(p.threads);
  const Lds16Net nd = lds16_net_of(net);
  return dispatch_cost_flags(h_inst[0].cost.affine != 0, h_inst[0].cost.need_control_cost != 0, [&](auto af, auto ct) {
    constexpr bool AF = decltype(af)::value, CT = decltype(ct)::value;
    if (fleet16_tiles_max(net) == 4) return fleet16_launch<&rollout_fleet16_kernel<4, AF, CT, 1024>>(grid, block, p.lds_bytes, stream, d_inst, n, nd);
    return fleet16_launch<&rollout_fleet16_kernel<8, AF, CT, kLds16MaxThreads8>>(grid, block, p.lds_bytes, stream, d_inst, n, nd);
  });
}

}  // namespace mppi
