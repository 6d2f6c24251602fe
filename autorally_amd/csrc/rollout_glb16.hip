// rollout_glb16.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) for gfx950, the form of EVERY layer list mppi_create accepts
// for the network model (3 <= n_layers <= 8, 6 in, 4 out, hidden widths 1..256): rollout_lds16_kernel's wave (wave16_step.hpp: one
// wavefront = 16 rollouts, the whole step in the wave on v_mfma_f32_16x16x4_f32, eps from the stand-alone generator, no rings, no
// riders, no barrier in the T loop; wave16_image.hpp: the walk over the image, shared with rollout_lds16.hip) with ONE change -- the
// image need not fit the LDS.  This file: the residency rule, the stream of a partly resident image, the kernel and the launcher:
//   * the image is lds16's, with up to 16 tiles per layer: compact bias quads, layer 0 half blocks (the "head", at most about
//     14 KB), then ONE stream of 1 KB blocks over all later layers in the order of their use, then kGlb16Ahead blocks of zeros;
//   * the head is always in LDS.  Of the stream the first R blocks are copied into LDS at the top of the kernel,
//       R = min(stream blocks (the zero blocks included), floor((160 KB - head bytes) / 1 KB), the cap given by name)
//     and block b is read with ds_read_b128 if b < R, else with global_load_dwordx4 from the image (default cache policy: every CU
//     re-reads the image every step, it stays in each XCD's L2).  The choice is wave-uniform and made per tile body, not per
//     load (wave16_image.hpp says why: kWave16Lds / Glb / Seam); lane l reads 16 B at 1024 b + 16 l either way;
//   * kGlb16Ahead blocks are always requested ahead of their use -- across pairs, layers and the resident / streamed seam: the
//     blocks at hand are a ring of kGlb16Ahead float4 with static indices, turned (wave16_turn) by the blocks a tile or pair of
//     tiles consumed, modulo the ring;
//   * arithmetic, lane map, padding rules and order are lds16's, unchanged: k ascending, one MFMA per k-step, C = +0, a padded
//     neuron's activation SET to 0, the bias after the chain -- bit-identical to "valu_lds" (oracle mode 1) and, on the lists
//     lds16 serves, to "lds16", for every R;
//   * instances: MTM = 8 tiles (lists up to 128 wide) and MTM = 16 (up to 256 wide: 64 activation and 64 accumulator registers).
// Below the launcher: the same kernel for a FLEET whose instances bring their own layer lists ("fleet_glb16").
#include "wave16_image.hpp"
#include "wave16_step.hpp"

namespace mppi {

constexpr size_t kGlb16MaxBytes = 160 * 1024;  // the dynamic-LDS limit the launcher requests
// waves per SIMD the workgroup rule counts with: registers per lane of the instances as DESIGN.md 4.16 records them (512 / allocation).
// Since the wave moved into wave16_step.hpp the 8-tile instance has 157-163 VGPRs and 3 would fit; the rule keeps
// counting with 2, which only under-counts what is resident, so every launch has the workgroup it had
constexpr int kGlb16WavesPerSimd8 = 2, kGlb16WavesPerSimd16 = 2;
// the largest workgroup of the instances = their __launch_bounds__.  The 16-tile instance has no scratch and no VGPR spill under 512
// at kGlb16Ahead = 2 (242-248 VGPRs); at 4 it needs 256 (tools/build_variant.sh ... -DMPPI_GLB16_AHEAD=4 -DMPPI_GLB16_T16=256)
#ifndef MPPI_GLB16_T16
#define MPPI_GLB16_T16 512
#endif
constexpr int kGlb16MaxThreads8 = 512, kGlb16MaxThreads16 = MPPI_GLB16_T16;

bool glb16_supported(const NetDesc &net) { return lds_list_ok(net, 256); }

// offsets and counts of a list glb16_supported accepts: lds16_net_of's answer with kGlb16Ahead zero blocks behind the stream
Lds16Net glb16_net_of(const NetDesc &net) { return wave16_image_net_of(net, kGlb16Ahead); }

int glb16_pack_floats(const NetDesc &net) { return glb16_supported(net) ? 4 * glb16_net_of(net).img_f4 : 0; }
// biases + layer 0: always resident
size_t glb16_head_bytes(const NetDesc &net) { return glb16_supported(net) ? 16 * (size_t)glb16_net_of(net).off[1] : 0; }
// the 1 KB blocks behind the head, the read-ahead's zero blocks included
int glb16_stream_blocks(const NetDesc &net)
{
  if (!glb16_supported(net)) return 0;
  const Lds16Net d = glb16_net_of(net);
  return (d.img_f4 - d.off[1]) / 64;
}
// R: the stream blocks a workgroup keeps in LDS; cap < 0: no cap by name
int glb16_resident_blocks(const NetDesc &net, int cap)
{
  if (!glb16_supported(net)) return 0;
  int r = glb16_stream_blocks(net);
  const int fit = (int)((kGlb16MaxBytes - glb16_head_bytes(net)) / 1024);
  r = fit < r ? fit : r;
  return (cap >= 0 && cap < r) ? cap : r;
}
// a workgroup's dynamic LDS: the head and the resident blocks
size_t glb16_lds_bytes(const NetDesc &net, int cap)
{
  return glb16_supported(net) ? glb16_head_bytes(net) + 1024 * (size_t)glb16_resident_blocks(net, cap) : 0;
}
size_t glb16_lds_limit() { return kGlb16MaxBytes; }

static int glb16_tiles_max(const NetDesc &net) { return wave16_image_tiles_max(net, 8); }  // 8 tiles (lists up to 128 wide) or 16

// The workgroup: wave16_image_block_threads' rule on the LDS this form requests -- the smaller of 256 / 512 threads for which
// every workgroup of the launch is resident at once, else the largest.
int glb16_block_threads(const NetDesc &net, int K, int cus, int cap)
{
  if (!glb16_supported(net) || K < kRolloutsPerWave || cus < 1) return 0;
  const bool wide = glb16_tiles_max(net) == 16;
  return wave16_image_block_threads(K, cus, glb16_lds_bytes(net, cap), kGlb16MaxBytes, wide ? kGlb16WavesPerSimd16 : kGlb16WavesPerSimd8,
                                    wide ? kGlb16MaxThreads16 : kGlb16MaxThreads8);
}

// The stream (wave16_image.hpp) of an image that is partly in LDS: where this lane's quad of stream block b is -- LDS below R,
// the image in global memory from R on (both pointers carry the lane).  The pointers are typed by their address space: two
// loads through generic pointers would be merged into ONE flat load of a selected address, which waits on both counters.
typedef const f32x4 __attribute__((address_space(3))) *Glb16LdsPtr;
typedef const f32x4 __attribute__((address_space(1))) *Glb16GlbPtr;
struct Glb16Stream {
  static constexpr int kAhead = kGlb16Ahead;
  static constexpr bool kResident = false;
  Glb16LdsPtr lds;
  Glb16GlbPtr glb;
  int R, b;  // the resident blocks; the cursor
  static __device__ __forceinline__ Glb16Stream at(const f32x4 *lds, const f32x4 *glb, const int R)
  {
    return Glb16Stream{(Glb16LdsPtr)lds, (Glb16GlbPtr)glb, R, 0};
  }
  // a body fetches all of its blocks from LDS, all from the image, or (the seam) picks per block
  __device__ __forceinline__ int mode(const int first, const int n) const
  {
    return (b + first + n - 1 < R) ? kWave16Lds : (b + first >= R) ? kWave16Glb : kWave16Seam;
  }
  template <int MODE>
  __device__ __forceinline__ f32x4 fetch(const int i) const
  {
    if (MODE == kWave16Lds || (MODE == kWave16Seam && b + i < R)) return lds[(b + i) * 64];  // wave-uniform: ds_read_b128
    return glb[(size_t)(b + i) * 64];                                                        // global_load_dwordx4
  }
  __device__ __forceinline__ void advance(const int n) { b += n; }
  // layer 0's 4 MTM existence masks are computed per step, not kept in (spilled) SGPR pairs: the 16-tile instance's SGPR pressure
  static __device__ __forceinline__ void keep_vector(int &lim) { asm volatile("" : "+v"(lim)); }
};

extern __shared__ __attribute__((aligned(16))) unsigned char glb16_smem[];

// R: the resident stream blocks, what the launcher sized the dynamic LDS for
template <int MTM, bool AFFINE, bool CTRL, int THREADS>
__global__ __launch_bounds__(THREADS) void rollout_glb16_kernel(const RolloutArgs a, const Lds16Net net, const int R_arg)
{
  f32x4 *const img = reinterpret_cast<f32x4 *>(glb16_smem);
  const f32x4 *const src = reinterpret_cast<const f32x4 *>(a.wpack);
  const int R = __builtin_amdgcn_readfirstlane(R_arg);
  {  // the head and the first R blocks of the stream into LDS: the image is in LDS order, 16 B per thread and pass
    const int n = net.off[1] + 64 * R;
    for (int q = threadIdx.x; q < n; q += blockDim.x) img[q] = src[q];
  }
  __syncthreads();  // the only barrier
  Wave16ImageNet<MTM, Glb16Stream> nn(img, src, net, R);
  wave16_rollout<AFFINE, CTRL>(a, nn);  // the step: wave16_step.hpp
}

hipError_t launch_rollout_glb16(const NetDesc &net, const RolloutArgs &a, int cus, int cap, hipStream_t stream)
{
  if (!glb16_supported(net) || a.K % 64 != 0 || a.gate != nullptr || cus < 1) return hipErrorInvalidValue;
  const int threads = glb16_block_threads(net, a.K, cus, cap);
  const int waves = a.K / kRolloutsPerWave, wpb = threads / 64;
  const dim3 grid((waves + wpb - 1) / wpb), block(threads);
  const int R = glb16_resident_blocks(net, cap);
  const size_t lds = glb16_lds_bytes(net, cap);
  if (lds > kGlb16MaxBytes) return hipErrorInvalidValue;
  const Lds16Net nd = glb16_net_of(net);
  return dispatch_cost_flags(a.cost.affine != 0, a.cost.need_control_cost != 0, [&](auto af, auto ct) {
    constexpr bool AF = decltype(af)::value, CT = decltype(ct)::value;
    if (glb16_tiles_max(net) == 8)
      return launch_wave16_image_instance<&rollout_glb16_kernel<8, AF, CT, kGlb16MaxThreads8>>(grid, block, lds, kGlb16MaxBytes, stream, a, nd, R);
    return launch_wave16_image_instance<&rollout_glb16_kernel<16, AF, CT, kGlb16MaxThreads16>>(grid, block, lds, kGlb16MaxBytes, stream, a, nd, R);
  });
}

// ---- "fleet_glb16": up to kMaxFleet independent controllers, EVERY ONE WITH ITS OWN LAYER LIST, in one launch ----
// The wave reads the layer list only as wave-uniform data and MTM only bounds the tile recursion and the register arrays, so an
// instance of the launch may bring its own list: workgroup (x, y) runs workgroup x of inst[y] on the list and the resident blocks
// of nets[y].  Both arrays are in DEVICE MEMORY, read-only behind __restrict__ pointers at a workgroup-uniform index: the block and
// the list arrive in scalar registers as kernel arguments do.  The list is used through a REFERENCE into the array -- a local copy
// of the struct is indexed at run time (net.boff[n_w - 1]) and would go to private memory.  One instance of the kernel serves a
// launch: 16 tiles if any list of the fleet is wider than 128, else 8; a narrower list leaves the upper tiles by the wave-uniform
// exits it leaves them by in a launch of its own, with the same bits.

FleetGlbNet fleet_glb16_net_of(const NetDesc &net, int cap)
{
  FleetGlbNet d{};
  if (!glb16_supported(net)) return d;
  d.net = glb16_net_of(net);
  d.R = glb16_resident_blocks(net, cap);
  return d;
}

// The plan of a launch: every instance keeps the R of a launch of its own (glb16_resident_blocks); the launch has ONE dynamic-LDS
// size, the largest of the instances', and ONE workgroup size, wave16_image_block_threads' rule with that LDS on the workgroups
// of the whole fleet (n = 1: glb16's own plan).  All zero for n outside 1..kMaxFleet, a K below one wave or a list glb16 refuses.
FleetGlb16Plan fleet_glb16_plan(const NetDesc *nets, const int *caps, const int *Ks, int n, int cus)
{
  FleetGlb16Plan p{};
  if (!nets || !caps || !Ks || n < 1 || n > kMaxFleet || cus < 1) return p;
  int kmax = 0, tiles = 8;
  size_t lds = 0;
  for (int i = 0; i < n; i++) {
    if (!glb16_supported(nets[i]) || Ks[i] < kRolloutsPerWave) return p;
    kmax = Ks[i] > kmax ? Ks[i] : kmax;
    tiles = glb16_tiles_max(nets[i]) > tiles ? 16 : tiles;
    const size_t b = glb16_lds_bytes(nets[i], caps[i]);
    lds = b > lds ? b : lds;
  }
  const bool wide = tiles == 16;
  p.tiles = tiles;
  p.lds_bytes = lds;
  p.threads = wave16_image_block_threads(Ks, n, cus, lds, kGlb16MaxBytes, wide ? kGlb16WavesPerSimd16 : kGlb16WavesPerSimd8,
                                         wide ? kGlb16MaxThreads16 : kGlb16MaxThreads8);
  const int wpb = p.threads / 64;
  p.grid_x = (kmax / kRolloutsPerWave + wpb - 1) / wpb;
  p.grid_y = n;
  return p;
}

template <int MTM, bool AFFINE, bool CTRL, int THREADS>
__global__ __launch_bounds__(THREADS) void rollout_fleet_glb16_kernel(const RolloutArgs *__restrict__ inst, const FleetGlbNet *__restrict__ nets, const int n)
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
  const Lds16Net &net = nets[blockIdx.y].net;  // a reference: see above
  const int R = __builtin_amdgcn_readfirstlane(nets[blockIdx.y].R);
  f32x4 *const img = reinterpret_cast<f32x4 *>(glb16_smem);
  const f32x4 *const src = reinterpret_cast<const f32x4 *>(a.wpack);
  {  // THIS instance's head and the first R blocks of its stream into LDS
    const int q_end = net.off[1] + 64 * R;
    for (int q = threadIdx.x; q < q_end; q += blockDim.x) img[q] = src[q];
  }
  __syncthreads();  // the only barrier
  Wave16ImageNet<MTM, Glb16Stream> nn(img, src, net, R);
  wave16_rollout<AFFINE, CTRL>(a, nn);  // the step: wave16_step.hpp (its absent waves of the last workgroup leave there)
}

template <auto KERN>
static hipError_t fleet_glb16_launch(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const RolloutArgs *d_inst, const FleetGlbNet *d_nets, int n)
{
  if (hipError_t e = raise_lds_limit_once<KERN>(kGlb16MaxBytes); e != hipSuccess) return e;
  MPPI_LAUNCH_ROLLOUT(KERN, grid, block, lds, stream, d_inst, d_nets, n);
  return hipGetLastError();
}

// nets / caps: every instance's layer list and the cap on its resident blocks (< 0: none); h_inst: the host's copy of the n argument
// blocks (K and the cost flags are read there); d_inst: the same blocks in device memory and d_nets: fleet_glb16_net_of(nets[i],
// caps[i]) of every instance there, both complete once `stream` reaches the launch.  Every instance: one pair (affine, control cost).
hipError_t launch_rollout_fleet_glb16(const NetDesc *nets, const int *caps, const RolloutArgs *h_inst, const RolloutArgs *d_inst, const FleetGlbNet *d_nets,
                                      int n, int cus, hipStream_t stream)
{
  if (!nets || !caps || !h_inst || !d_inst || !d_nets || n < 1 || n > kMaxFleet) return hipErrorInvalidValue;
  int Ks[kMaxFleet];
  for (int i = 0; i < n; i++) {
    const RolloutArgs &a = h_inst[i];
    if (a.K % 64 != 0 || a.gate != nullptr || a.cost.affine != h_inst[0].cost.affine || a.cost.need_control_cost != h_inst[0].cost.need_control_cost)
      return hipErrorInvalidValue;
    Ks[i] = a.K;
  }
  const FleetGlb16Plan p = fleet_glb16_plan(nets, caps, Ks, n, cus);
  if (p.threads == 0 || p.lds_bytes > kGlb16MaxBytes) return hipErrorInvalidValue;
  const dim3 grid(p.grid_x, p.grid_y), block(p.threads);
  return dispatch_cost_flags(h_inst[0].cost.affine != 0, h_inst[0].cost.need_control_cost != 0, [&](auto af, auto ct) {
    constexpr bool AF = decltype(af)::value, CT = decltype(ct)::value;
    if (p.tiles == 8)
      return fleet_glb16_launch<&rollout_fleet_glb16_kernel<8, AF, CT, kGlb16MaxThreads8>>(grid, block, p.lds_bytes, stream, d_inst, d_nets, n);
    return fleet_glb16_launch<&rollout_fleet_glb16_kernel<16, AF, CT, kGlb16MaxThreads16>>(grid, block, p.lds_bytes, stream, d_inst, d_nets, n);
  });
}

}  // namespace mppi
