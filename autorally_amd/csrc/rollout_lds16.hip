// rollout_lds16.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) for gfx950, the THROUGHPUT form of any layer list with hidden
// widths up to 128 whose image fits the LDS: rollout_mfma_kernel (rollout_mfma.hip) -- one wavefront = 16 rollouts, the whole step
// in the wave, eps from the stand-alone generator, no rings, no riders, no barrier in the T loop -- with the layer list a kernel
// ARGUMENT and the A operands of v_mfma_f32_16x16x4_f32 read from an LDS image instead of kept in registers:
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
//   * register indices are static: the loops over tiles and input tiles are unrolled for MTM = 4 (lists up to 64 wide) or 8
//     tiles with wave-uniform exits, so a narrow list does not pay 64 accumulator and activation registers.
// Image (pack_lds16_weights, abi_pack.hip; Lds16Net below has the offsets), in float4 ("quads"):
//   biases    weight layer j < n_w - 1: 4 MT_j quads, quad 4 m + g = kTanhScale x (b[16 m + g], b[16 m + 4 + g], b[16 m + 8 + g],
//             b[16 m + 12 + g]) (0 where the neuron does not exist) -- read as a broadcast; then ONE quad b_out[0..3]
//   layer 0   MT_0 half blocks of 32 quads: float2 of lane (row, kk) of tile m = (W[n][kk], W[n][4 + kk]) (0 for k >= 6), n = 16 m +
//             4 (row & 3) + (row >> 2)
//   layer j   the stream: for every pair P of tiles, for mi = 0 .. MT_(j-1) - 1: block (2 P, mi), block (2 P + 1, mi); then for an
//             odd last tile: block (MT_j - 1, mi), mi ascending.  Output layer: one tile, neuron of row = row & 3
//   then kLds16Ahead blocks of zeros (the read-ahead behind the last layer)
#include "mppi_kernels.hpp"

namespace mppi {

constexpr size_t kLds16MaxBytes = 160 * 1024;  // the dynamic-LDS limit the launcher requests
constexpr int kLds16Ahead = 2;                 // blocks requested ahead of their use
// registers per lane of the instances (ISA) as waves per SIMD (512 / allocation): what the workgroup rule counts with
constexpr int kLds16WavesPerSimd4 = 4, kLds16WavesPerSimd8 = 3;
constexpr int kLds16MaxThreads8 = 512;         // the largest workgroup of the 8-tile instance

// offsets and counts of a list lds_list_ok(net, 128) accepts
Lds16Net lds16_net_of(const NetDesc &net)
{
  Lds16Net d{};
  d.n_w = net.n_layers - 1;
  int q = 0;
  for (int j = 0; j < d.n_w; j++) {
    const bool last = j == d.n_w - 1;
    d.nout[j] = net.layers[j + 1];
    d.mt[j] = last ? 1 : (net.layers[j + 1] + 15) / 16;
    d.ks[j] = j == 0 ? 2 : 4 * d.mt[j - 1];
    d.boff[j] = q;
    q += last ? 1 : 4 * d.mt[j];
  }
  for (int j = 0; j < d.n_w; j++) {
    d.off[j] = q;
    q += j == 0 ? 32 * d.mt[0] : 64 * d.mt[j] * d.mt[j - 1];
  }
  d.img_f4 = q + 64 * kLds16Ahead;
  return d;
}

int lds16_pack_floats(const NetDesc &net) { return lds_list_ok(net, 128) ? 4 * lds16_net_of(net).img_f4 : 0; }
// a workgroup's dynamic LDS: the image and nothing else; 0 for a list the form does not take whatever its size
size_t lds16_lds_bytes(const NetDesc &net) { return sizeof(float) * (size_t)lds16_pack_floats(net); }
size_t lds16_lds_limit() { return kLds16MaxBytes; }
bool lds16_supported(const NetDesc &net) { return lds_list_ok(net, 128) && lds16_lds_bytes(net) <= kLds16MaxBytes; }

static int lds16_tiles_max(const NetDesc &net)
{
  int w = 0;
  for (int l = 1; l + 1 < net.n_layers; l++) w = net.layers[l] > w ? net.layers[l] : w;
  return w <= 64 ? 4 : 8;
}

// The workgroup: the image is per workgroup, so small workgroups spread a modest K over all CUs and a big image leaves one
// workgroup per CU -- the smallest of 256 / 512 / 1024 threads for which every workgroup of the launch is resident at once
// (LDS: floor(limit / image) workgroups per CU; registers: the instance's waves per SIMD), else the largest the instance has.
int lds16_block_threads(const NetDesc &net, int K, int cus)
{
  if (!lds16_supported(net) || K < kRolloutsPerWave || cus < 1) return 0;
  const bool wide = lds16_tiles_max(net) == 8;
  const int waves = K / kRolloutsPerWave, wps = wide ? kLds16WavesPerSimd8 : kLds16WavesPerSimd4;
  const int largest = wide ? kLds16MaxThreads8 : 1024;
  const int by_lds = (int)(kLds16MaxBytes / lds16_lds_bytes(net));
  for (int threads = 256; threads <= largest; threads *= 2) {
    const int wpb = threads / 64, by_regs = 4 * wps / wpb;
    const int per_cu = by_lds < by_regs ? by_lds : by_regs;
    if ((waves + wpb - 1) / wpb <= (long long)per_cu * cus) return threads;
  }
  return largest;
}

#define MPPI_L16_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_16x16x4f32((A), (B), (C), 0, 0, 0)

// a pair of tiles: stream blocks 2 MI and 2 MI + 1 are input tile MI of d0 and of d1 -- the same B operands, the k-steps of the
// two independent chains alternate.  w: the two blocks at hand; p: the pair's first block (this lane's quad)
template <int MTM, int MI>
__device__ __forceinline__ void lds16_pair(f32x4 &d0, f32x4 &d1, const float (&act)[MTM * 4], f32x4 (&w)[2], const f32x4 *p, const int mt_in)
{
  if constexpr (MI < MTM) {
    if (MI > 0 && MI >= mt_in) return;  // wave-uniform
    const f32x4 x0 = w[0], x1 = w[1];
    w[0] = p[(MI + 1) * 128];
    w[1] = p[(MI + 1) * 128 + 64];
    lds_pin_reads();
    d0 = MPPI_L16_MFMA(x0[0], act[4 * MI + 0], d0);
    d1 = MPPI_L16_MFMA(x1[0], act[4 * MI + 0], d1);
    d0 = MPPI_L16_MFMA(x0[1], act[4 * MI + 1], d0);
    d1 = MPPI_L16_MFMA(x1[1], act[4 * MI + 1], d1);
    d0 = MPPI_L16_MFMA(x0[2], act[4 * MI + 2], d0);
    d1 = MPPI_L16_MFMA(x1[2], act[4 * MI + 2], d1);
    d0 = MPPI_L16_MFMA(x0[3], act[4 * MI + 3], d0);
    d1 = MPPI_L16_MFMA(x1[3], act[4 * MI + 3], d1);
    lds16_pair<MTM, MI + 1>(d0, d1, act, w, p, mt_in);
  }
}

// one tile (an odd last tile, the output layer): stream block MI is input tile MI of d; the blocks at hand alternate between
// w[0] and w[1] (lds16_single puts the next one back into w[0])
template <int MTM, int MI>
__device__ __forceinline__ void lds16_single_step(f32x4 &d, const float (&act)[MTM * 4], f32x4 (&w)[2], const f32x4 *p, const int mt_in)
{
  if constexpr (MI < MTM) {
    if (MI > 0 && MI >= mt_in) return;  // wave-uniform
    const f32x4 x = w[MI & 1];
    w[MI & 1] = p[(MI + 2) * 64];
    lds_pin_reads();
    d = MPPI_L16_MFMA(x[0], act[4 * MI + 0], d);
    d = MPPI_L16_MFMA(x[1], act[4 * MI + 1], d);
    d = MPPI_L16_MFMA(x[2], act[4 * MI + 2], d);
    d = MPPI_L16_MFMA(x[3], act[4 * MI + 3], d);
    lds16_single_step<MTM, MI + 1>(d, act, w, p, mt_in);
  }
}
template <int MTM>
__device__ __forceinline__ void lds16_single(f32x4 &d, const float (&act)[MTM * 4], f32x4 (&w)[2], const f32x4 *p, const int mt_in)
{
  lds16_single_step<MTM, 0>(d, act, w, p, mt_in);
  if (mt_in & 1) {  // wave-uniform
    const f32x4 x = w[0];
    w[0] = w[1];
    w[1] = x;
  }
}

// D[mt_out tiles] = W x act over mt_in input tiles; p: the layer's first block, moved behind its last
template <int MTM>
__device__ __forceinline__ void lds16_layer(f32x4 (&acc)[MTM], const float (&act)[MTM * 4], f32x4 (&w)[2], const f32x4 *&p, const int mt_out,
                                            const int mt_in)
{
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int P = 0; P < MTM / 2; P++) {
    if (2 * P >= mt_out) break;  // wave-uniform
    acc[2 * P] = zero4;
    if (2 * P + 1 < mt_out) {
      acc[2 * P + 1] = zero4;
      lds16_pair<MTM, 0>(acc[2 * P], acc[2 * P + 1], act, w, p, mt_in);
      p += 128 * mt_in;
    } else {
      lds16_single<MTM>(acc[2 * P], act, w, p, mt_in);
      p += 64 * mt_in;
    }
  }
}

// act = tanh(acc + bias) of a hidden layer of nout neurons; pb: quad 4 m + g of the layer's biases is pb[4 m]; lim = nout - g
template <int MTM>
__device__ __forceinline__ void lds16_tanh(const f32x4 (&acc)[MTM], float (&act)[MTM * 4], const f32x4 *pb, const int mt, const int lim)
{
#pragma unroll
  for (int m = 0; m < MTM; m++) {
    if (m > 0 && m >= mt) break;  // wave-uniform
    const f32x4 b = pb[4 * m];
    const f32x2 v0 = tanh_bias2(f32x2{acc[m][0], acc[m][1]}, f32x2{b[0], b[1]});
    const f32x2 v1 = tanh_bias2(f32x2{acc[m][2], acc[m][3]}, f32x2{b[2], b[3]});
    act[4 * m + 0] = (16 * m + 0 < lim) ? v0.x : 0.0f;  // neuron 16 m + 4 r + g exists
    act[4 * m + 1] = (16 * m + 4 < lim) ? v0.y : 0.0f;
    act[4 * m + 2] = (16 * m + 8 < lim) ? v1.x : 0.0f;
    act[4 * m + 3] = (16 * m + 12 < lim) ? v1.y : 0.0f;
  }
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
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (wave * kRolloutsPerWave >= a.K) return;  // whole wave (K is a multiple of 64)
  const int j = lane & 15, g = lane >> 4;
  const int k = wave * kRolloutsPerWave + j;

  // per weight layer i, bits 8 i .. 8 i + 7: its outputs - 1 -- the T loop reads no kernel argument
  const int n_w = __builtin_amdgcn_readfirstlane(net.n_w);
  unsigned long long lay = 0;
#pragma unroll
  for (int i = 0; i < 7; i++) lay |= (unsigned long long)((net.nout[i] - 1) & 255) << (8 * i);
  const int nout0 = (int)(lay & 255) + 1, mt0 = (nout0 + 15) >> 4;
  const f32x4 *const pb0 = img + g;                                                   // this row group's bias quads, layer 0
  const f32x4 *const pbo = img + net.boff[n_w - 1];                                   // b_out
  const f32x2 *const p0 = reinterpret_cast<const f32x2 *>(img + net.off[0]) + lane;  // layer 0: half blocks
  const f32x4 *const p1 = img + net.off[1] + lane;                                   // the stream

  float s[kStateDim];
#pragma unroll
  for (int i = 0; i < kStateDim; i++) s[i] = a.state[i];
  int crash = 0;
  float J = 0.0f;

  const int K = a.K, T = a.T;
  float2 *const noise = reinterpret_cast<float2 *>(a.noise);
  const float2 *const Useq = reinterpret_cast<const float2 *>(a.U);
  const bool noise_free_k = (k == 0);       // mppi_controller.cu:136
  const bool pure_noise_k = (k >= a.k99);   // :141, k >= .99*NUM_ROLLOUTS in double (host)

  // rollout_mfma_kernel's step: everything a step reads from global memory is requested one step ahead, the step is cut into
  // scheduling regions in which the MFMAs of one network piece run next to independent cost / kinematics arithmetic
  float2 eps = noise[(size_t)k];            // t = 0
  float2 Unext = Useq[0];
  double rt_next = a.inv_t[0];
  for (int t = 0; t < T; t++) {
    // ---- region 1: controls, layer 0, sin/cos, costmap addresses and fetches ----
    // layer 0's operands and the first two blocks of the stream, requested in front of the control arithmetic
    f32x2 w0[MTM];
#pragma unroll
    for (int m = 0; m < MTM; m++) {
      if (m > 0 && m >= mt0) break;  // wave-uniform
      w0[m] = p0[m * 64];
    }
    f32x4 w[2];
    w[0] = p1[0];
    w[1] = p1[64];
    lds_pin_reads();
    const float2 e = eps;
    const float2 Ut = Unext;
    const double rt = rt_next;
    const int tn = min(t + 1, T - 1);
    eps = noise[(size_t)tn * K + k];
    Unext = Useq[tn];
    rt_next = a.inv_t[tn];
    // control perturbation, mppi_controller.cu:136-153
    const bool nf = noise_free_k | (t < a.opt_delay);
    const float n0 = e.x * a.nu[0], n1 = e.y * a.nu[1];
    const float du0 = nf ? 0.0f : n0, du1 = nf ? 0.0f : n1;
    float u0 = nf ? Ut.x : (pure_noise_k ? n0 : Ut.x + n0);
    float u1 = nf ? Ut.y : (pure_noise_k ? n1 : Ut.y + n1);
    // stored before the clamp (Q3); the four lanes of a rollout write the same value
    noise[(size_t)t * K + k] = make_float2(u0, u1);
    u0 = clampf(u0, a.u_lo[0], a.u_hi[0]);
    u1 = clampf(u1, a.u_lo[1], a.u_hi[1]);
    f32x4 acc[MTM];
    float act[MTM * 4];
    {
      const float b0 = (g == 0) ? s[3] : (g == 1) ? s[4] : (g == 2) ? s[5] : s[6];
      const float b1 = (g == 0) ? u0 : (g == 1) ? u1 : 0.0f;
#pragma unroll
      for (int m = 0; m < MTM; m++) {
        if (m > 0 && m >= mt0) break;  // wave-uniform
        f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        z = MPPI_L16_MFMA(w0[m].x, b0, z);
        acc[m] = MPPI_L16_MFMA(w0[m].y, b1, z);
      }
    }
    float spsi, cpsi;
    sincos_fast(s[2], spsi, cpsi);
    float tf, tb;
    track_fetch<AFFINE>(a.cost, s, cpsi, spsi, tf, tb);
    __builtin_amdgcn_sched_barrier(0);

    // ---- region 2: hidden layers next to kinematics and the texel-free cost terms ----
    int mt_in = mt0, lim = nout0 - g;
    const f32x4 *p = p1, *pb = pb0;
    for (int i = 1; i < n_w - 1; i++) {
      lds16_tanh<MTM>(acc, act, pb, mt_in, lim);
      pb += 4 * mt_in;
      const int nout = (int)((lay >> (8 * i)) & 255) + 1, mt_out = (nout + 15) >> 4;
      lds16_layer<MTM>(acc, act, w, p, mt_out, mt_in);
      mt_in = mt_out;
      lim = nout - g;
    }
    float sd[kStateDim];
    sd[0] = fmaf(cpsi, s[4], -(spsi * s[5]));  // computeKinematics, neural_net_model.cu:346-355
    sd[1] = fmaf(spsi, s[4], cpsi * s[5]);
    sd[2] = a.negate_yaw_der ? -s[6] : s[6];
    CostTerms ct;
    cost_terms_a<CTRL>(a.cost, a.nu, s[4], s[5], u0, u1, du0, du1, ct);
    __builtin_amdgcn_sched_barrier(0);

    // ---- region 3: output layer next to the track / crash terms and the running mean ----
    float d[4];
    {
      const f32x4 bo = pbo[0];
      lds16_tanh<MTM>(acc, act, pb, mt_in, lim);
      f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
      lds16_single<MTM>(o, act, w, p, mt_in);
#pragma unroll
      for (int r = 0; r < 4; r++) d[r] = o[r] + bo[r];  // the bias after the chain, as in the reference
    }
    {
      // running mean over t = 1..T-1 of the cost of the state before the update (Q5); the
      // t = 0 evaluation is computed and discarded
      int crash_new = crash;
      const float c = cost_terms_b(a.cost, ct, tf, tb, crash_new);
      const float Jn = running_mean(J, c, t, rt);
      J = (t > 0) ? Jn : J;
      crash = (t > 0) ? crash_new : crash;
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- region 4: incrementState (:334-344) and getCrash (costs.cu:301-305) ----
    sd[3] = d[0]; sd[4] = d[1]; sd[5] = d[2]; sd[6] = d[3];
#pragma unroll
    for (int i = 0; i < kStateDim; i++) s[i] = fmaf(sd[i], a.dt, s[i]);
    crash |= (int)(fabsf(s[3]) >= kRollCrash);
  }
  if (g == 0) a.costs[k] = J + 0.0f;  // + terminalCost (= 0), costs.cu:411-414
}
#undef MPPI_L16_MFMA

template <auto KERN>
static hipError_t launch_lds16_instance(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const RolloutArgs &a, const Lds16Net &nd)
{
  if (hipError_t e = raise_lds_limit_once<KERN>(kLds16MaxBytes); e != hipSuccess) return e;
  MPPI_LAUNCH_ROLLOUT(KERN, grid, block, lds, stream, a, nd);
  return hipGetLastError();
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
    if (lds16_tiles_max(net) == 4) return launch_lds16_instance<&rollout_lds16_kernel<4, AF, CT, 1024>>(grid, block, lds, stream, a, nd);
    return launch_lds16_instance<&rollout_lds16_kernel<8, AF, CT, kLds16MaxThreads8>>(grid, block, lds, stream, a, nd);
  });
}

}  // namespace mppi
