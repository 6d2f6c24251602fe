// rollout_glb16.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) for gfx950, the form of EVERY layer list mppi_create accepts
// for the network model (3 <= n_layers <= 8, 6 in, 4 out, hidden widths 1..256): rollout_lds16_kernel's wave (rollout_lds16.hip:
// one wavefront = 16 rollouts, the whole step in the wave on v_mfma_f32_16x16x4_f32, eps from the stand-alone generator, no rings,
// no riders, no barrier in the T loop) with ONE change -- the image need not fit the LDS:
//   * the image is lds16's, with up to 16 tiles per layer: compact bias quads, layer 0 half blocks (the "head", at most about
//     14 KB), then ONE stream of 1 KB blocks over all later layers in the order of their use, then kGlb16Ahead blocks of zeros;
//   * the head is always in LDS.  Of the stream the first R blocks are copied into LDS at the top of the kernel,
//       R = min(stream blocks (the zero blocks included), floor((160 KB - head bytes) / 1 KB), the cap given by name)
//     and block b is read with ds_read_b128 if b < R, else with global_load_dwordx4 from the image (default cache policy: every CU
//     re-reads the image every step, it stays in each XCD's L2).  The choice is wave-uniform and made per tile body, not per
//     load (glb16_mode below says why); lane l reads 16 B at 1024 b + 16 l either way;
//   * kGlb16Ahead blocks are always requested ahead of their use -- across pairs, layers and the resident / streamed seam: the
//     blocks at hand are a ring of kGlb16Ahead float4 with static indices, turned (glb16_turn) by the blocks a tile or pair of
//     tiles consumed, modulo the ring;
//   * arithmetic, lane map, padding rules and order are lds16's, unchanged: k ascending, one MFMA per k-step, C = +0, a padded
//     neuron's activation SET to 0, the bias after the chain -- bit-identical to "valu_lds" (oracle mode 1) and, on the lists
//     lds16 serves, to "lds16", for every R;
//   * instances: MTM = 8 tiles (lists up to 128 wide) and MTM = 16 (up to 256 wide: 64 activation and 64 accumulator registers).
#include "mppi_kernels.hpp"

namespace mppi {

constexpr size_t kGlb16MaxBytes = 160 * 1024;  // the dynamic-LDS limit the launcher requests
// registers per lane of the instances (ISA) as waves per SIMD (512 / allocation): what the workgroup rule counts with
constexpr int kGlb16WavesPerSimd8 = 2, kGlb16WavesPerSimd16 = 2;
// the largest workgroup of the instances = their __launch_bounds__.  The 16-tile instance has no scratch and no VGPR spill under 512
// at kGlb16Ahead = 2 (242-248 VGPRs); at 4 it needs 256 (tools/build_variant.sh ... -DMPPI_GLB16_AHEAD=4 -DMPPI_GLB16_T16=256)
#ifndef MPPI_GLB16_T16
#define MPPI_GLB16_T16 512
#endif
constexpr int kGlb16MaxThreads8 = 512, kGlb16MaxThreads16 = MPPI_GLB16_T16;

bool glb16_supported(const NetDesc &net) { return lds_list_ok(net, 256); }

// offsets and counts of a list glb16_supported accepts: lds16_net_of's answer with kGlb16Ahead zero blocks behind the stream
Lds16Net glb16_net_of(const NetDesc &net)
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
  d.img_f4 = q + 64 * kGlb16Ahead;
  return d;
}

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

static int glb16_tiles_max(const NetDesc &net)
{
  int w = 0;
  for (int l = 1; l + 1 < net.n_layers; l++) w = net.layers[l] > w ? net.layers[l] : w;
  return w <= 128 ? 8 : 16;
}

// The workgroup: lds16_block_threads' rule on the LDS this form requests -- the smallest of 256 / 512 threads for which every
// workgroup of the launch is resident at once (LDS: floor(limit / requested bytes) workgroups per CU; registers: the
// instance's waves per SIMD), else the largest.
int glb16_block_threads(const NetDesc &net, int K, int cus, int cap)
{
  if (!glb16_supported(net) || K < kRolloutsPerWave || cus < 1) return 0;
  const int waves = K / kRolloutsPerWave, wps = glb16_tiles_max(net) == 8 ? kGlb16WavesPerSimd8 : kGlb16WavesPerSimd16;
  const int by_lds = (int)(kGlb16MaxBytes / glb16_lds_bytes(net, cap));
  const int largest = glb16_tiles_max(net) == 8 ? kGlb16MaxThreads8 : kGlb16MaxThreads16;
  for (int threads = 256; threads <= largest; threads *= 2) {
    const int wpb = threads / 64, by_regs = 4 * wps / wpb;
    const int per_cu = by_lds < by_regs ? by_lds : by_regs;
    if ((waves + wpb - 1) / wpb <= (long long)per_cu * cus) return threads;
  }
  return largest;
}

#define MPPI_G16_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_16x16x4f32((A), (B), (C), 0, 0, 0)

// where this lane's quad of stream block b is: LDS below R, the image in global memory from R on (both pointers carry the lane).
// The pointers are typed by their address space: two loads through generic pointers would be merged into ONE flat load of a
// selected address, which waits on both counters.
typedef const f32x4 __attribute__((address_space(3))) *Glb16LdsPtr;
typedef const f32x4 __attribute__((address_space(1))) *Glb16GlbPtr;
struct Glb16Stream {
  Glb16LdsPtr lds;
  Glb16GlbPtr glb;
  int R;
};
// How a tile's (or a pair's) fetches are issued.  A wait count is an immediate, and a counted wait for a block is right only if
// the kind of every younger fetch is known where the code is compiled: a fetch that picks its kind at run time makes every wait
// behind it a wait for ALL outstanding loads.  So the body of a tile exists three times -- all of its fetches resident, all
// streamed, and (once per step, the seam) the choice per block -- and the tile picks one (glb16_mode: blocks ascend within a step,
// so a streamed fetch is never followed by a resident one before the next step).
enum { kGlb16Lds = 0, kGlb16Glb = 1, kGlb16Seam = 2 };
template <int MODE>
__device__ __forceinline__ f32x4 glb16_fetch(const Glb16Stream &st, const int b)
{
  if (MODE == kGlb16Lds || (MODE == kGlb16Seam && b < st.R)) return st.lds[b * 64];  // wave-uniform: ds_read_b128
  return st.glb[(size_t)b * 64];                                                      // global_load_dwordx4
}
// of a body that consumes blocks b .. b + n - 1 and so fetches blocks b + kGlb16Ahead .. b + n - 1 + kGlb16Ahead
__device__ __forceinline__ int glb16_mode(const Glb16Stream &st, const int b, const int n)
{
  return (b + n - 1 + kGlb16Ahead < st.R) ? kGlb16Lds : (b + kGlb16Ahead >= st.R) ? kGlb16Glb : kGlb16Seam;
}
// behind a seam body: its fetches have landed (what the compiler knows about them is the same on every path again)
__device__ __forceinline__ void glb16_land(f32x4 (&w)[kGlb16Ahead])
{
#pragma unroll
  for (int i = 0; i < kGlb16Ahead; i++) asm volatile("" : "+v"(w[i]));
}

// the ring of blocks at hand turned left by r blocks (wave-uniform, 0 <= r < kGlb16Ahead): w[0] is the next block again
__device__ __forceinline__ void glb16_turn(f32x4 (&w)[kGlb16Ahead], const int r)
{
  static_assert(kGlb16Ahead == 2 || kGlb16Ahead == 4, "the ring is 2 or 4 blocks");
  if (r & 1) {
    const f32x4 x = w[0];
#pragma unroll
    for (int i = 0; i + 1 < kGlb16Ahead; i++) w[i] = w[i + 1];
    w[kGlb16Ahead - 1] = x;
  }
  if constexpr (kGlb16Ahead == 4) {
    if (r & 2) {
      const f32x4 x0 = w[0], x1 = w[1];
      w[0] = w[2];
      w[1] = w[3];
      w[2] = x0;
      w[3] = x1;
    }
  }
}

// a pair of tiles: stream blocks b + 2 MI and b + 2 MI + 1 are input tile MI of d0 and of d1 -- the same B operands, the k-steps
// of the two independent chains alternate.  w: the ring, w[0] = block b
template <int MTM, int MODE, int MI>
__device__ __forceinline__ void glb16_pair_step(f32x4 &d0, f32x4 &d1, const float (&act)[MTM * 4], f32x4 (&w)[kGlb16Ahead],
                                                const Glb16Stream &st, const int b, const int mt_in)
{
  if constexpr (MI < MTM) {
    if (MI > 0 && MI >= mt_in) return;  // wave-uniform
    constexpr int s0 = (2 * MI) % kGlb16Ahead, s1 = (2 * MI + 1) % kGlb16Ahead;
    const f32x4 x0 = w[s0], x1 = w[s1];
    w[s0] = glb16_fetch<MODE>(st, b + 2 * MI + kGlb16Ahead);
    w[s1] = glb16_fetch<MODE>(st, b + 2 * MI + kGlb16Ahead + 1);
    lds_pin_reads();
    d0 = MPPI_G16_MFMA(x0[0], act[4 * MI + 0], d0);
    d1 = MPPI_G16_MFMA(x1[0], act[4 * MI + 0], d1);
    d0 = MPPI_G16_MFMA(x0[1], act[4 * MI + 1], d0);
    d1 = MPPI_G16_MFMA(x1[1], act[4 * MI + 1], d1);
    d0 = MPPI_G16_MFMA(x0[2], act[4 * MI + 2], d0);
    d1 = MPPI_G16_MFMA(x1[2], act[4 * MI + 2], d1);
    d0 = MPPI_G16_MFMA(x0[3], act[4 * MI + 3], d0);
    d1 = MPPI_G16_MFMA(x1[3], act[4 * MI + 3], d1);
    glb16_pair_step<MTM, MODE, MI + 1>(d0, d1, act, w, st, b, mt_in);
  }
}
template <int MTM>
__device__ __forceinline__ void glb16_pair(f32x4 &d0, f32x4 &d1, const float (&act)[MTM * 4], f32x4 (&w)[kGlb16Ahead], const Glb16Stream &st,
                                           int &b, const int mt_in)
{
  const int mode = glb16_mode(st, b, 2 * mt_in);  // wave-uniform
  if (mode == kGlb16Lds) glb16_pair_step<MTM, kGlb16Lds, 0>(d0, d1, act, w, st, b, mt_in);
  else if (mode == kGlb16Glb) glb16_pair_step<MTM, kGlb16Glb, 0>(d0, d1, act, w, st, b, mt_in);
  else {
    glb16_pair_step<MTM, kGlb16Seam, 0>(d0, d1, act, w, st, b, mt_in);
    glb16_land(w);
  }
  b += 2 * mt_in;
  glb16_turn(w, (2 * mt_in) & (kGlb16Ahead - 1));
}

// one tile (an odd last tile, the output layer): stream block b + MI is input tile MI of d
template <int MTM, int MODE, int MI>
__device__ __forceinline__ void glb16_single_step(f32x4 &d, const float (&act)[MTM * 4], f32x4 (&w)[kGlb16Ahead], const Glb16Stream &st,
                                                  const int b, const int mt_in)
{
  if constexpr (MI < MTM) {
    if (MI > 0 && MI >= mt_in) return;  // wave-uniform
    constexpr int s = MI % kGlb16Ahead;
    const f32x4 x = w[s];
    w[s] = glb16_fetch<MODE>(st, b + MI + kGlb16Ahead);
    lds_pin_reads();
    d = MPPI_G16_MFMA(x[0], act[4 * MI + 0], d);
    d = MPPI_G16_MFMA(x[1], act[4 * MI + 1], d);
    d = MPPI_G16_MFMA(x[2], act[4 * MI + 2], d);
    d = MPPI_G16_MFMA(x[3], act[4 * MI + 3], d);
    glb16_single_step<MTM, MODE, MI + 1>(d, act, w, st, b, mt_in);
  }
}
template <int MTM>
__device__ __forceinline__ void glb16_single(f32x4 &d, const float (&act)[MTM * 4], f32x4 (&w)[kGlb16Ahead], const Glb16Stream &st, int &b,
                                             const int mt_in)
{
  const int mode = glb16_mode(st, b, mt_in);  // wave-uniform
  if (mode == kGlb16Lds) glb16_single_step<MTM, kGlb16Lds, 0>(d, act, w, st, b, mt_in);
  else if (mode == kGlb16Glb) glb16_single_step<MTM, kGlb16Glb, 0>(d, act, w, st, b, mt_in);
  else {
    glb16_single_step<MTM, kGlb16Seam, 0>(d, act, w, st, b, mt_in);
    glb16_land(w);
  }
  b += mt_in;
  glb16_turn(w, mt_in & (kGlb16Ahead - 1));
}

// D[mt_out tiles] = W x act over mt_in input tiles; b: the layer's first block, moved behind its last.  The pairs are walked by
// recursion: a loop of this size is past what "#pragma unroll" unrolls, and acc[] indexed by a loop counter would live in scratch
template <int MTM, int P>
__device__ __forceinline__ void glb16_tiles(f32x4 (&acc)[MTM], const float (&act)[MTM * 4], f32x4 (&w)[kGlb16Ahead], const Glb16Stream &st, int &b,
                                            const int mt_out, const int mt_in)
{
  if constexpr (P < MTM / 2) {
    if (2 * P >= mt_out) return;  // wave-uniform
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    acc[2 * P] = zero4;
    if (2 * P + 1 < mt_out) {
      acc[2 * P + 1] = zero4;
      glb16_pair<MTM>(acc[2 * P], acc[2 * P + 1], act, w, st, b, mt_in);
    } else {
      glb16_single<MTM>(acc[2 * P], act, w, st, b, mt_in);
    }
    glb16_tiles<MTM, P + 1>(acc, act, w, st, b, mt_out, mt_in);
  }
}
template <int MTM>
__device__ __forceinline__ void glb16_layer(f32x4 (&acc)[MTM], const float (&act)[MTM * 4], f32x4 (&w)[kGlb16Ahead], const Glb16Stream &st, int &b,
                                            const int mt_out, const int mt_in)
{
  glb16_tiles<MTM, 0>(acc, act, w, st, b, mt_out, mt_in);
}

// act = tanh(acc + bias) of a hidden layer of nout neurons; pb: quad 4 m + g of the layer's biases is pb[4 m]; lim = nout - g
template <int MTM>
__device__ __forceinline__ void glb16_tanh(const f32x4 (&acc)[MTM], float (&act)[MTM * 4], const f32x4 *pb, const int mt, const int lim)
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
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (wave * kRolloutsPerWave >= a.K) return;  // whole wave (K is a multiple of 64)
  const int j = lane & 15, g = lane >> 4;
  const int k = wave * kRolloutsPerWave + j;

  // per weight layer i, bits 8 i .. 8 i + 7: its outputs - 1 (256 fits) -- the T loop reads no kernel argument
  const int n_w = __builtin_amdgcn_readfirstlane(net.n_w);
  unsigned long long lay = 0;
#pragma unroll
  for (int i = 0; i < 7; i++) lay |= (unsigned long long)((net.nout[i] - 1) & 255) << (8 * i);
  const int nout0 = (int)(lay & 255) + 1, mt0 = (nout0 + 15) >> 4;
  const f32x4 *const pb0 = img + g;                                                   // this row group's bias quads, layer 0
  const f32x4 *const pbo = img + net.boff[n_w - 1];                                   // b_out
  const f32x2 *const p0 = reinterpret_cast<const f32x2 *>(img + net.off[0]) + lane;  // layer 0: half blocks
  const Glb16Stream st = {(Glb16LdsPtr)(img + net.off[1] + lane), (Glb16GlbPtr)(src + net.off[1] + lane), R};  // the stream

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

  // rollout_lds16_kernel's step
  float2 eps = noise[(size_t)k];            // t = 0
  float2 Unext = Useq[0];
  double rt_next = a.inv_t[0];
  for (int t = 0; t < T; t++) {
    // ---- region 1: controls, layer 0, sin/cos, costmap addresses and fetches ----
    // layer 0's operands and the first blocks of the stream, requested in front of the control arithmetic
    f32x2 w0[MTM];
#pragma unroll
    for (int m = 0; m < MTM; m++) {
      if (m > 0 && m >= mt0) break;  // wave-uniform
      w0[m] = p0[m * 64];
    }
    f32x4 w[kGlb16Ahead];
    if (R >= kGlb16Ahead) {  // wave-uniform
#pragma unroll
      for (int i = 0; i < kGlb16Ahead; i++) w[i] = glb16_fetch<kGlb16Lds>(st, i);
    } else if (R == 0) {
#pragma unroll
      for (int i = 0; i < kGlb16Ahead; i++) w[i] = glb16_fetch<kGlb16Glb>(st, i);
    } else {
#pragma unroll
      for (int i = 0; i < kGlb16Ahead; i++) w[i] = glb16_fetch<kGlb16Seam>(st, i);
      glb16_land(w);
    }
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
        z = MPPI_G16_MFMA(w0[m].x, b0, z);
        acc[m] = MPPI_G16_MFMA(w0[m].y, b1, z);
      }
    }
    float spsi, cpsi;
    sincos_fast(s[2], spsi, cpsi);
    float tf, tb;
    track_fetch<AFFINE>(a.cost, s, cpsi, spsi, tf, tb);
    __builtin_amdgcn_sched_barrier(0);

    // ---- region 2: hidden layers next to kinematics and the texel-free cost terms ----
    int mt_in = mt0, lim = nout0 - g, b = 0;
    asm volatile("" : "+v"(lim));  // layer 0's 4 MTM existence masks are computed per step, not kept in (spilled) SGPR pairs
    const f32x4 *pb = pb0;
    for (int i = 1; i < n_w - 1; i++) {
      glb16_tanh<MTM>(acc, act, pb, mt_in, lim);
      pb += 4 * mt_in;
      const int nout = (int)((lay >> (8 * i)) & 255) + 1, mt_out = (nout + 15) >> 4;
      glb16_layer<MTM>(acc, act, w, st, b, mt_out, mt_in);
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
      glb16_tanh<MTM>(acc, act, pb, mt_in, lim);
      f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
      glb16_single<MTM>(o, act, w, st, b, mt_in);
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
#undef MPPI_G16_MFMA

template <auto KERN>
static hipError_t launch_glb16_instance(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const RolloutArgs &a, const Lds16Net &nd, int R)
{
  if (hipError_t e = raise_lds_limit_once<KERN>(kGlb16MaxBytes); e != hipSuccess) return e;
  MPPI_LAUNCH_ROLLOUT(KERN, grid, block, lds, stream, a, nd, R);
  return hipGetLastError();
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
    if (glb16_tiles_max(net) == 8) return launch_glb16_instance<&rollout_glb16_kernel<8, AF, CT, kGlb16MaxThreads8>>(grid, block, lds, stream, a, nd, R);
    return launch_glb16_instance<&rollout_glb16_kernel<16, AF, CT, kGlb16MaxThreads16>>(grid, block, lds, stream, a, nd, R);
  });
}

}  // namespace mppi
