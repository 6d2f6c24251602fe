// wave16_image.hpp -- the network of the wave (wave16_step.hpp) read from an IMAGE with the layer list a kernel argument, shared
// by rollout_lds16.hip (the whole image in LDS) and rollout_glb16.hip (the image partly streamed from global memory).  Here,
// once: the image's offsets (Lds16Net), the workgroup rule and the launch of an instance on the host; on the device the walk
// over the image's one stream of 1 KB blocks -- pairs of tiles, single tiles, a layer -- the tanh with the padded-neuron rule
// and the wave's network policy (Wave16ImageNet).  The layout and the order of the image are described in rollout_lds16.hip.
// A form adds its STREAM, a cursor over the blocks behind the head (this lane's quad of each):
//   S::kAhead               blocks requested ahead of their use = the ring of blocks at hand (2 or 4)
//   S::kResident            every block is in LDS: only the resident body of a tile exists
//   S::at(lds, glb, R)      the cursor at block 0; lds / glb: this lane's quad of block 0 in LDS / in the image in global memory
//   cur.mode(first, n)      how blocks first .. first + n - 1 from the cursor are fetched (wave-uniform; not of a kResident stream)
//   cur.fetch<MODE>(i)      this lane's quad of block i from the cursor
//   cur.advance(n)          the cursor n blocks on
//   S::keep_vector(lim)     what the form wants to hold against the register allocator's choice (nothing, as a rule)
#pragma once
#include "mppi_kernels.hpp"

namespace mppi {

// offsets and counts of a list lds_list_ok accepts, `ahead` blocks of zeros behind the stream
inline Lds16Net wave16_image_net_of(const NetDesc &net, int ahead)
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
  d.img_f4 = q + 64 * ahead;
  return d;
}

// the instance of a list: `small` tiles per layer while no hidden layer is wider than 16 x small, else twice as many
inline int wave16_image_tiles_max(const NetDesc &net, int small)
{
  int w = 0;
  for (int l = 1; l + 1 < net.n_layers; l++) w = net.layers[l] > w ? net.layers[l] : w;
  return w <= 16 * small ? small : 2 * small;
}

// The workgroup: the image is per workgroup, so small workgroups spread a modest K over all CUs and a big image leaves one
// workgroup per CU -- the smallest of 256 / 512 / .. / largest threads for which every workgroup of the launch is resident at
// once (LDS: floor(limit / requested bytes) workgroups per CU; registers: the instance's waves per SIMD), else the largest.
// Several instances in one launch (rollout_fleet16.hip): a workgroup serves one instance, so the launch's workgroups are the sum
// of the instances' own.
inline int wave16_image_block_threads(const int *Ks, int n, int cus, size_t lds_bytes, size_t lds_limit, int waves_per_simd, int largest)
{
  const int by_lds = (int)(lds_limit / lds_bytes);
  for (int threads = 256; threads <= largest; threads *= 2) {
    const int wpb = threads / 64, by_regs = 4 * waves_per_simd / wpb;
    const int per_cu = by_lds < by_regs ? by_lds : by_regs;
    long long blocks = 0;
    for (int i = 0; i < n; i++) blocks += (Ks[i] / kRolloutsPerWave + wpb - 1) / wpb;
    if (blocks <= (long long)per_cu * cus) return threads;
  }
  return largest;
}
inline int wave16_image_block_threads(int K, int cus, size_t lds_bytes, size_t lds_limit, int waves_per_simd, int largest)
{
  return wave16_image_block_threads(&K, 1, cus, lds_bytes, lds_limit, waves_per_simd, largest);
}

// extra: the kernel's arguments behind the layer list
template <auto KERN, class... Extra>
inline hipError_t launch_wave16_image_instance(dim3 grid, dim3 block, size_t lds, size_t lds_limit, hipStream_t stream, const RolloutArgs &a,
                                               const Lds16Net &nd, Extra... extra)
{
  if (hipError_t e = raise_lds_limit_once<KERN>(lds_limit); e != hipSuccess) return e;
  MPPI_LAUNCH_ROLLOUT(KERN, grid, block, lds, stream, a, nd, extra...);
  return hipGetLastError();
}

#define MPPI_W16_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_16x16x4f32((A), (B), (C), 0, 0, 0)

// How a tile's (or a pair's) fetches are issued.  A wait count is an immediate, and a counted wait for a block is right only if
// the kind of every younger fetch is known where the code is compiled: a fetch that picks its kind at run time makes every wait
// behind it a wait for ALL outstanding loads.  So the body of a tile exists three times -- all of its fetches resident, all
// streamed, and (once per step, the seam) the choice per block -- and the tile picks one (blocks ascend within a step, so a
// streamed fetch is never followed by a resident one before the next step).  A stream that is always resident has the first only.
enum { kWave16Lds = 0, kWave16Glb = 1, kWave16Seam = 2 };
template <int MODE>
using Wave16Mode = std::integral_constant<int, MODE>;

// behind a seam body: its fetches have landed (what the compiler knows about them is the same on every path again)
template <int AHEAD>
__device__ __forceinline__ void wave16_land(f32x4 (&w)[AHEAD])
{
#pragma unroll
  for (int i = 0; i < AHEAD; i++) asm volatile("" : "+v"(w[i]));
}

// body(Wave16Mode<MODE>) for the mode of the fetches of blocks first .. first + n - 1 from the cursor into the ring w
template <class S, class F>
__device__ __forceinline__ void wave16_by_mode(const S &cur, f32x4 (&w)[S::kAhead], const int first, const int n, F &&body)
{
  if constexpr (S::kResident) {
    body(Wave16Mode<kWave16Lds>{});
  } else {
    const int mode = cur.mode(first, n);  // wave-uniform
    if (mode == kWave16Lds) body(Wave16Mode<kWave16Lds>{});
    else if (mode == kWave16Glb) body(Wave16Mode<kWave16Glb>{});
    else {
      body(Wave16Mode<kWave16Seam>{});
      wave16_land(w);
    }
  }
}

// the ring of blocks at hand turned left by r blocks (wave-uniform, 0 <= r < AHEAD): w[0] is the next block again
template <int AHEAD>
__device__ __forceinline__ void wave16_turn(f32x4 (&w)[AHEAD], const int r)
{
  static_assert(AHEAD == 2 || AHEAD == 4, "the ring is 2 or 4 blocks");
  if (r & 1) {
    const f32x4 x = w[0];
#pragma unroll
    for (int i = 0; i + 1 < AHEAD; i++) w[i] = w[i + 1];
    w[AHEAD - 1] = x;
  }
  if constexpr (AHEAD == 4) {
    if (r & 2) {
      const f32x4 x0 = w[0], x1 = w[1];
      w[0] = w[2];
      w[1] = w[3];
      w[2] = x0;
      w[3] = x1;
    }
  }
}

// the ring filled with the first blocks from the cursor (the top of a step)
template <class S>
__device__ __forceinline__ void wave16_fill(f32x4 (&w)[S::kAhead], const S &cur)
{
  wave16_by_mode(cur, w, 0, S::kAhead, [&](auto m) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < S::kAhead; i++) w[i] = cur.template fetch<decltype(m)::value>(i);
  });
}

// a pair of tiles: blocks 2 MI and 2 MI + 1 from the cursor are input tile MI of d0 and of d1 -- the same B operands, the k-steps
// of the two independent chains alternate.  w: the ring, w[0] = the block at the cursor
template <int MTM, int MODE, int MI, class S>
__device__ __forceinline__ void wave16_pair_step(f32x4 &d0, f32x4 &d1, const float (&act)[MTM * 4], f32x4 (&w)[S::kAhead], const S &cur,
                                                 const int mt_in)
{
  if constexpr (MI < MTM) {
    if (MI > 0 && MI >= mt_in) return;  // wave-uniform
    constexpr int s0 = (2 * MI) % S::kAhead, s1 = (2 * MI + 1) % S::kAhead;
    const f32x4 x0 = w[s0], x1 = w[s1];
    w[s0] = cur.template fetch<MODE>(2 * MI + S::kAhead);
    w[s1] = cur.template fetch<MODE>(2 * MI + S::kAhead + 1);
    lds_pin_reads();
    d0 = MPPI_W16_MFMA(x0[0], act[4 * MI + 0], d0);
    d1 = MPPI_W16_MFMA(x1[0], act[4 * MI + 0], d1);
    d0 = MPPI_W16_MFMA(x0[1], act[4 * MI + 1], d0);
    d1 = MPPI_W16_MFMA(x1[1], act[4 * MI + 1], d1);
    d0 = MPPI_W16_MFMA(x0[2], act[4 * MI + 2], d0);
    d1 = MPPI_W16_MFMA(x1[2], act[4 * MI + 2], d1);
    d0 = MPPI_W16_MFMA(x0[3], act[4 * MI + 3], d0);
    d1 = MPPI_W16_MFMA(x1[3], act[4 * MI + 3], d1);
    wave16_pair_step<MTM, MODE, MI + 1>(d0, d1, act, w, cur, mt_in);
  }
}
template <int MTM, class S>
__device__ __forceinline__ void wave16_pair(f32x4 &d0, f32x4 &d1, const float (&act)[MTM * 4], f32x4 (&w)[S::kAhead], S &cur, const int mt_in)
{
  wave16_by_mode(cur, w, S::kAhead, 2 * mt_in, [&](auto m) __attribute__((always_inline)) {
    wave16_pair_step<MTM, decltype(m)::value, 0>(d0, d1, act, w, cur, mt_in);
  });
  cur.advance(2 * mt_in);
  wave16_turn(w, (2 * mt_in) & (S::kAhead - 1));
}

// one tile (an odd last tile, the output layer): block MI from the cursor is input tile MI of d
template <int MTM, int MODE, int MI, class S>
__device__ __forceinline__ void wave16_single_step(f32x4 &d, const float (&act)[MTM * 4], f32x4 (&w)[S::kAhead], const S &cur, const int mt_in)
{
  if constexpr (MI < MTM) {
    if (MI > 0 && MI >= mt_in) return;  // wave-uniform
    constexpr int s = MI % S::kAhead;
    const f32x4 x = w[s];
    w[s] = cur.template fetch<MODE>(MI + S::kAhead);
    lds_pin_reads();
    d = MPPI_W16_MFMA(x[0], act[4 * MI + 0], d);
    d = MPPI_W16_MFMA(x[1], act[4 * MI + 1], d);
    d = MPPI_W16_MFMA(x[2], act[4 * MI + 2], d);
    d = MPPI_W16_MFMA(x[3], act[4 * MI + 3], d);
    wave16_single_step<MTM, MODE, MI + 1>(d, act, w, cur, mt_in);
  }
}
template <int MTM, class S>
__device__ __forceinline__ void wave16_single(f32x4 &d, const float (&act)[MTM * 4], f32x4 (&w)[S::kAhead], S &cur, const int mt_in)
{
  wave16_by_mode(cur, w, S::kAhead, mt_in, [&](auto m) __attribute__((always_inline)) {
    wave16_single_step<MTM, decltype(m)::value, 0>(d, act, w, cur, mt_in);
  });
  cur.advance(mt_in);
  wave16_turn(w, mt_in & (S::kAhead - 1));
}

// D[mt_out tiles] = W x act over mt_in input tiles; the cursor: the layer's first block, moved behind its last.  The pairs are
// walked by recursion: a loop of this size is past what "#pragma unroll" unrolls, and acc[] indexed by a loop counter would live
// in scratch
template <int MTM, int P, class S>
__device__ __forceinline__ void wave16_tiles(f32x4 (&acc)[MTM], const float (&act)[MTM * 4], f32x4 (&w)[S::kAhead], S &cur, const int mt_out,
                                             const int mt_in)
{
  if constexpr (P < MTM / 2) {
    if (2 * P >= mt_out) return;  // wave-uniform
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    acc[2 * P] = zero4;
    if (2 * P + 1 < mt_out) {
      acc[2 * P + 1] = zero4;
      wave16_pair<MTM>(acc[2 * P], acc[2 * P + 1], act, w, cur, mt_in);
    } else {
      wave16_single<MTM>(acc[2 * P], act, w, cur, mt_in);
    }
    wave16_tiles<MTM, P + 1>(acc, act, w, cur, mt_out, mt_in);
  }
}

// act = tanh(acc + bias) of a hidden layer of nout neurons; pb: quad 4 m + g of the layer's biases is pb[4 m]; lim = nout - g
template <int MTM>
__device__ __forceinline__ void wave16_tanh(const f32x4 (&acc)[MTM], float (&act)[MTM * 4], const f32x4 *pb, const int mt, const int lim)
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

// The wave's network (wave16_step.hpp) of an instance of MTM tiles per layer.  img: the head and the resident blocks in LDS; src:
// the image in global memory; R: the resident blocks of the stream (a stream that is always resident reads neither src nor R)
template <int MTM, class S>
struct Wave16ImageNet {
  struct Step {
    f32x2 w0[MTM];       // layer 0's half blocks
    f32x4 w[S::kAhead];  // the ring of blocks at hand
    S cur;               // the stream from the next block to use on
    f32x4 acc[MTM];
    float act[MTM * 4];
    int mt_in, lim;      // of the layer in acc: its tiles, its outputs - g
    const f32x4 *pb;     // and its bias quads
  };
  f32x4 *const img;
  const f32x4 *const src;
  const Lds16Net &net;
  const int R;
  int n_w, nout0, mt0;
  unsigned long long lay;  // per weight layer i, bits 8 i .. 8 i + 7: its outputs - 1 (256 fits) -- the T loop reads no kernel argument
  const f32x4 *pb0, *pbo;  // this row group's bias quads of layer 0; b_out
  const f32x2 *p0;         // layer 0: half blocks
  S first;                 // the stream at block 0

  __device__ __forceinline__ Wave16ImageNet(f32x4 *img_, const f32x4 *src_, const Lds16Net &net_, int R_) : img(img_), src(src_), net(net_), R(R_) {}

  __device__ __forceinline__ void load(const int lane)
  {
    n_w = __builtin_amdgcn_readfirstlane(net.n_w);
    lay = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) lay |= (unsigned long long)((net.nout[i] - 1) & 255) << (8 * i);
    nout0 = (int)(lay & 255) + 1;
    mt0 = (nout0 + 15) >> 4;
    pb0 = img + (lane >> 4);
    pbo = img + net.boff[n_w - 1];
    p0 = reinterpret_cast<const f32x2 *>(img + net.off[0]) + lane;
    first = S::at(img + net.off[1] + lane, src + net.off[1] + lane, R);
  }

  // layer 0's operands and the first blocks of the stream
  __device__ __forceinline__ void request(Step &x) const
  {
#pragma unroll
    for (int m = 0; m < MTM; m++) {
      if (m > 0 && m >= mt0) break;  // wave-uniform
      x.w0[m] = p0[m * 64];
    }
    x.cur = first;
    wave16_fill(x.w, x.cur);
    lds_pin_reads();
  }

  __device__ __forceinline__ void layer0(Step &x, const int g, const float s3, const float s4, const float s5, const float s6, const float u0,
                                         const float u1) const
  {
    const float b0 = (g == 0) ? s3 : (g == 1) ? s4 : (g == 2) ? s5 : s6;
    const float b1 = (g == 0) ? u0 : (g == 1) ? u1 : 0.0f;
#pragma unroll
    for (int m = 0; m < MTM; m++) {
      if (m > 0 && m >= mt0) break;  // wave-uniform
      f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
      z = MPPI_W16_MFMA(x.w0[m].x, b0, z);
      x.acc[m] = MPPI_W16_MFMA(x.w0[m].y, b1, z);
    }
  }

  __device__ __forceinline__ void hidden(Step &x, const int g) const
  {
    int mt_in = mt0, lim = nout0 - g;
    S::keep_vector(lim);
    const f32x4 *pb = pb0;
    for (int i = 1; i < n_w - 1; i++) {
      wave16_tanh<MTM>(x.acc, x.act, pb, mt_in, lim);
      pb += 4 * mt_in;
      const int nout = (int)((lay >> (8 * i)) & 255) + 1, mt_out = (nout + 15) >> 4;
      wave16_tiles<MTM, 0>(x.acc, x.act, x.w, x.cur, mt_out, mt_in);
      mt_in = mt_out;
      lim = nout - g;
    }
    x.mt_in = mt_in;
    x.lim = lim;
    x.pb = pb;
  }

  __device__ __forceinline__ void output(Step &x, float (&d)[4]) const
  {
    const f32x4 bo = pbo[0];
    wave16_tanh<MTM>(x.acc, x.act, x.pb, x.mt_in, x.lim);
    f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
    wave16_single<MTM>(o, x.act, x.w, x.cur, x.mt_in);
#pragma unroll
    for (int r = 0; r < 4; r++) d[r] = o[r] + bo[r];  // the bias after the chain, as in the reference
  }
};
#undef MPPI_W16_MFMA

// ---- the image that is in LDS as a whole (rollout_lds16.hip, rollout_fleet16.hip) ----
constexpr size_t kLds16MaxBytes = 160 * 1024;  // the dynamic-LDS limit the launcher requests
constexpr int kLds16Ahead = 2;                 // blocks requested ahead of their use
// registers per lane of the instances (ISA) as waves per SIMD (512 / allocation): what the workgroup rule counts with
constexpr int kLds16WavesPerSimd4 = 4, kLds16WavesPerSimd8 = 3;
constexpr int kLds16MaxThreads8 = 512;         // the largest workgroup of the 8-tile instance

// the stream (wave16_image.hpp) of an image that is in LDS as a whole: a pointer to this lane's quad of the next block to use.
// With two blocks ahead a pair leaves the ring as it found it and an odd tile count swaps w[0] and w[1]
struct Lds16Stream {
  static constexpr int kAhead = kLds16Ahead;
  static constexpr bool kResident = true;
  const f32x4 *p;
  static __device__ __forceinline__ Lds16Stream at(const f32x4 *lds, const f32x4 *, int) { return Lds16Stream{lds}; }
  template <int MODE>
  __device__ __forceinline__ f32x4 fetch(const int i) const { return p[i * 64]; }
  __device__ __forceinline__ void advance(const int n) { p += 64 * n; }
  static __device__ __forceinline__ void keep_vector(int &) {}
};

}  // namespace mppi
