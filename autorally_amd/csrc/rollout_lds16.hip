// rollout_lds16.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) for gfx950, the THROUGHPUT form of any layer list with hidden
// widths up to 128 whose image fits the LDS: the 16x16x4 wave (wave16_step.hpp: one wavefront = 16 rollouts, the whole step in the
// wave, eps from the stand-alone generator, no rings, no riders, no barrier in the T loop) with the layer list a kernel ARGUMENT
// and the A operands of v_mfma_f32_16x16x4_f32 read from an LDS image (wave16_image.hpp: the walk over the image, shared with
// rollout_glb16.hip) instead of kept in registers.  This file: the capacity rule, the kernel and the launcher (the stream of an image
// that is in LDS as a whole, Lds16Stream, is in wave16_image.hpp: rollout_fleet16.hip runs the same wave).  Layout and order:
//   * lane l = (rollout j = l & 15, k-slot / row group g = l >> 4).  A hidden layer of nout outputs is MT = ceil(nout / 16) M tiles
//     with an accumulator (4 registers) each; D row 16 m + 4 g + r carries neuron 16 m + 4 r + g (the row permutation of
//     pack_mfma_weights, per tile), which is k-slot g of k-step 4 m + r of the next layer: a layer's D registers are the next
//     layer's B operands, no cross-lane traffic.  A layer's inputs are the 4 MT k-steps of the layer in front (layer 0: two,
//     [s3, s4, s5, s6][g] and [u0, u1, 0, 0][g]); every accumulator sees k ascending, C = 0, the bias afterwards: the fmaf chain
//     of neural_net_model.cu:379-394, so the form is bit-identical to "valu_lds" (oracle mode 1);
//   * a neuron that does not exist (the padding of the last tile) has zero weights and a zero bias and its activation is SET to
//     0 (its zero weights times an infinite state entry would be NaN, which the next layer's padded k-steps would spread); a
//     padded k-step adds fma(0, 0, d) = d to an accumulator that started at +0 and never is -0;
//   * one ds_read_b128 feeds FOUR consecutive k-steps of one M tile -- a "block": 64 lanes x 16 B, lane (row, kk) holds
//     W[neuron of row][16 mi + 4 c + kk], c = 0..3, for input tile mi.  The tiles of a layer are walked in PAIRS whose k-steps
//     alternate in the instruction stream (two independent chains: a dependent 16x16x4 pair issues 8 cycles late); an odd last
//     tile and the output layer (one tile, rows = output row & 3, as nn_last) are one dependent chain;
//   * the blocks lie in the image in the order of their use, ONE stream over all layers, and two blocks are always requested
//     ahead of their use (across pairs and layers too; the first two of layer 1 at the top of the step);
//   * register indices are static: the walks over tiles and input tiles are unrolled for MTM = 4 (lists up to 64 wide) or 8
//     tiles with wave-uniform exits, so a narrow list does not pay 64 accumulator and activation registers.
// Image (pack_lds16_weights, abi_pack.hip; Lds16Net has the offsets: wave16_image_net_of), in float4 ("quads"):
//   biases    weight layer j < n_w - 1: 4 MT_j quads, quad 4 m + g = kTanhScale x (b[16 m + g], b[16 m + 4 + g], b[16 m + 8 + g],
//             b[16 m + 12 + g]) (0 where the neuron does not exist) -- read as a broadcast; then ONE quad b_out[0..3]
//   layer 0   MT_0 half blocks of 32 quads: float2 of lane (row, kk) of tile m = (W[n][kk], W[n][4 + kk]) (0 for k >= 6), n = 16 m +
//             4 (row & 3) + (row >> 2)
//   layer j   the stream: for every pair P of tiles, for mi = 0 .. MT_(j-1) - 1: block (2 P, mi), block (2 P + 1, mi); then for an
//             odd last tile: block (MT_j - 1, mi), mi ascending.  Output layer: one tile, neuron of row = row & 3
//   then kLds16Ahead blocks of zeros (the read-ahead behind the last layer)
#include "wave16_image.hpp"
#include "wave16_step.hpp"

namespace mppi {

// offsets and counts of a list lds_list_ok(net, 128) accepts
Lds16Net lds16_net_of(const NetDesc &net) { return wave16_image_net_of(net, kLds16Ahead); }

int lds16_pack_floats(const NetDesc &net) { return lds_list_ok(net, 128) ? 4 * lds16_net_of(net).img_f4 : 0; }
// a workgroup's dynamic LDS: the image and nothing else; 0 for a list the form does not take whatever its size
size_t lds16_lds_bytes(const NetDesc &net) { return sizeof(float) * (size_t)lds16_pack_floats(net); }
size_t lds16_lds_limit() { return kLds16MaxBytes; }
bool lds16_supported(const NetDesc &net) { return lds_list_ok(net, 128) && lds16_lds_bytes(net) <= kLds16MaxBytes; }

static int lds16_tiles_max(const NetDesc &net) { return wave16_image_tiles_max(net, 4); }  // 4 tiles (lists up to 64 wide) or 8

// The workgroup: wave16_image_block_threads' rule on the image -- the smallest of 256 / 512 / 1024 threads for which every
// workgroup of the launch is resident at once, else the largest the instance has.
int lds16_block_threads(const NetDesc &net, int K, int cus)
{
  if (!lds16_supported(net) || K < kRolloutsPerWave || cus < 1) return 0;
  const bool wide = lds16_tiles_max(net) == 8;
  return wave16_image_block_threads(K, cus, lds16_lds_bytes(net), kLds16MaxBytes, wide ? kLds16WavesPerSimd8 : kLds16WavesPerSimd4,
                                    wide ? kLds16MaxThreads8 : 1024);
}

extern __shared__ __attribute__((aligned(16))) unsigned char lds16_smem[];

template <int MTM, bool AFFINE, bool CTRL, int THREADS>
__global__ __launch_bounds__(THREADS) void rollout_lds16_kernel(const RolloutArgs a, const Lds16Net net)
{
  f32x4 *const img = reinterpret_cast<f32x4 *>(lds16_smem);
  {  // the image into LDS: it is in LDS order, 16 B per thread and pass
    const f32x4 *src = reinterpret_cast<const f32x4 *>(a.wpack);
    for (int q = threadIdx.x; q < net.img_f4; q += blockDim.x) img[q] = src[q];
  }
  __syncthreads();  // the only barrier
  Wave16ImageNet<MTM, Lds16Stream> nn(img, reinterpret_cast<const f32x4 *>(a.wpack), net, 0);
  wave16_rollout<AFFINE, CTRL>(a, nn);  // the step: wave16_step.hpp
}

hipError_t launch_rollout_lds16(const NetDesc &net, const RolloutArgs &a, int cus, hipStream_t stream)
{
  if (!lds16_supported(net) || a.K % 64 != 0 || a.gate != nullptr || cus < 1) return hipErrorInvalidValue;
  const int threads = lds16_block_threads(net, a.K, cus);
  const int waves = a.K / kRolloutsPerWave, wpb = threads / 64;
  const dim3 grid((waves + wpb - 1) / wpb), block(threads);
  const size_t lds = lds16_lds_bytes(net);
  const Lds16Net nd = lds16_net_of(net);
  return dispatch_cost_flags(a.cost.affine != 0, a.cost.need_control_cost != 0, [&](auto af, auto ct) {
    constexpr bool AF = decltype(af)::value, CT = decltype(ct)::value;
    if (lds16_tiles_max(net) == 4)
      return launch_wave16_image_instance<&rollout_lds16_kernel<4, AF, CT, 1024>>(grid, block, lds, kLds16MaxBytes, stream, a, nd);
    return launch_wave16_image_instance<&rollout_lds16_kernel<8, AF, CT, kLds16MaxThreads8>>(grid, block, lds, kLds16MaxBytes, stream, a, nd);
  });
}

}  // namespace mppi
