// rollout_glb44.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) for gfx950, the LATENCY form of EVERY layer list mppi_create
// accepts for the network model (3 <= n_layers <= 8, 6 in, 4 out, hidden widths 1..256): rollout_lds128.hip's group (m44_group.hpp:
// 512 threads per 16 rollouts, four dynamics waves of four rollouts on v_mfma_f32_4x4x1 with A-matrix broadcast, the riders, the
// record rings, one barrier, the gate) on a PARTLY RESIDENT image (rollout_glb16.hip's residency):
//   * a hidden layer of nout outputs is H = ceil(nout / 64) in 1..4 "halves": half h holds neurons 64 h .. 64 h + 63 in its own
//     accumulator d[h] (a lane is neuron 64 h + lane); its up to 256 inputs are up to four transposed activation sets: quad q of
//     k-steps takes its A operand from set q >> 4, ABID = q & 15.  Every accumulator sees k = 0 .. nin - 1 ascending, one
//     instruction per step from +0, the bias after the chain: the fmaf chain of neural_net_model.cu:379-394, so the form is
//     bit-identical to "valu_lds" (oracle mode 1), to "lds128" / "lds44" on the lists they serve and to "glb16", for every R;
//   * the steps of the H chains alternate in the instruction stream (lds128_chain2); a layer never enters the code of halves it
//     does not have; the OUTPUT layer is one more chain of up to 64 quads into ONE accumulator, row c at lane 16 c;
//   * a lane without a neuron in the first hidden layer has its activation SET to 0, in every half (its zero weights times an
//     infinite state entry are NaN);
//   * the image (pack_glb44_weights, abi_pack.hip) in 1 KB quads, float4 q of lane l at float4 index q * 64 + l: kGlb44BiasQuads
//     bias quads (quad j, float h: bias of neuron 64 h + l of weight layer j, hidden layers x kTanhScale; output layer, float 0:
//     b_out[l >> 4]), then per weight layer ceil(nin / 4) x H quads interleaved in the order of their use (quad q' H + h =
//     W[64 h + l][4 q' .. 4 q' + 3]), the output layer's row c at lane 16 c, then kGlb44Ahead quads of zeros;
//   * the HEAD (bias quads + layer 0) is always in LDS (layer 0 in registers over the T loop).  Of the stream behind it the first
//       R = min(stream quads (the zero quads included), floor((160 KB - kM44GroupImageOffset - head bytes) / 1 KB), the cap by name)
//     quads are copied into LDS behind the group's shared state; quad b is read with ds_read_b128 if b < R, else with
//     global_load_dwordx4 from the image (it stays in each XCD's L2), the two pointers typed by their address space;
//   * the choice is wave-uniform and made per BODY, not per load (wave16_image.hpp: kWave16Lds / Glb / Seam says why).  One body is one input
//     set (up to 16 quads of k-steps) of one layer, instantiated per (H, resident | streamed | seam); the set's A operand is
//     chosen by a wave-uniform select in front of it;
//   * quads are always requested ahead of their use -- across bodies, layers and the seam: a ring of kGlb44Ahead float4 with static
//     indices, turned by what a body consumed modulo the ring.  Resident quads are requested kGlb44AheadLds ahead (lds128's depth:
//     measured 7 % faster than the streamed depth on a resident list), streamed ones kGlb44Ahead; the step's one seam body fills the
//     ring from the one depth to the other.
#include "m44_group.hpp"

namespace mppi {

constexpr size_t kGlb44MaxBytes = 160 * 1024;  // the dynamic-LDS limit the launcher requests
constexpr int kGlb44A = kGlb44Ahead;      // the ring: quads requested ahead of their use while they are streamed
constexpr int kGlb44AL = kGlb44AheadLds;  // ... while they are resident (lds128's depth): the ring is only this deep then
static_assert(kGlb44A >= 2 && kGlb44A <= 16 && kGlb44AL >= 1 && kGlb44AL <= kGlb44A, "the ring is 2 .. 16 quads, the resident depth at most the ring");

__host__ __device__ inline int glb44_quads_of(int nin) { return (nin + 3) >> 2; }
__host__ __device__ inline int glb44_halves_of(int nout) { return (nout + 63) >> 6; }

bool glb44_supported(const NetDesc &net) { return lds_list_ok(net, 256); }

// bias quads + layer 0: always resident
static int glb44_head_quads(const NetDesc &net) { return kGlb44BiasQuads + 2 * glb44_halves_of(net.layers[1]); }
size_t glb44_head_bytes(const NetDesc &net) { return glb44_supported(net) ? 1024 * (size_t)glb44_head_quads(net) : 0; }
// the 1 KB quads behind the head, the read-ahead's zero quads included
int glb44_stream_quads(const NetDesc &net)
{
  if (!glb44_supported(net)) return 0;
  const int n_w = net.n_layers - 1;
  int q = kGlb44Ahead;
  for (int j = 1; j < n_w; j++) q += glb44_quads_of(net.layers[j]) * (j + 1 < n_w ? glb44_halves_of(net.layers[j + 1]) : 1);
  return q;
}
int glb44_pack_floats(const NetDesc &net) { return glb44_supported(net) ? 256 * (glb44_head_quads(net) + glb44_stream_quads(net)) : 0; }
// R: the stream quads a group keeps in LDS; cap < 0: no cap by name
int glb44_resident_quads(const NetDesc &net, int cap)
{
  if (!glb44_supported(net)) return 0;
  int r = glb44_stream_quads(net);
  const int fit = (int)((kGlb44MaxBytes - kM44GroupImageOffset - glb44_head_bytes(net)) / 1024);
  r = fit < r ? fit : r;
  return (cap >= 0 && cap < r) ? cap : r;
}
// the group's dynamic LDS: shared state, head, resident quads
size_t glb44_lds_bytes(const NetDesc &net, int cap)
{
  return glb44_supported(net) ? kM44GroupImageOffset + glb44_head_bytes(net) + 1024 * (size_t)glb44_resident_quads(net, cap) : 0;
}
size_t glb44_lds_limit() { return kGlb44MaxBytes; }

// where this lane's float4 of stream quad b is (rollout_glb16.hip: Glb16Stream): both pointers carry the lane
typedef const m44_f4 __attribute__((address_space(3))) *Glb44LdsPtr;
typedef const m44_f4 __attribute__((address_space(1))) *Glb44GlbPtr;
struct Glb44Stream {
  Glb44LdsPtr lds;
  Glb44GlbPtr glb;
  int R;
};
enum { kGlb44Lds = 0, kGlb44Glb = 1, kGlb44Seam = 2 };
template <int MODE>
__device__ __forceinline__ m44_f4 glb44_fetch(const Glb44Stream &st, const int b)
{
  if (MODE == kGlb44Lds || (MODE == kGlb44Seam && b < st.R)) return st.lds[b * 64];  // wave-uniform: ds_read_b128
  return st.glb[(size_t)b * 64];                                                      // global_load_dwordx4
}
// of a body that consumes quads b .. b + n - 1.  While the ring is shallow (kGlb44AL quads at hand) a body whose fetches b + kGlb44AL
// .. b + n - 1 + kGlb44AL are all resident is a resident one; the first body for which they are not is THE seam body of the step:
// it fills the ring to kGlb44A quads and fetches kGlb44A ahead, the choice per quad; behind it (deep) every fetch is b + kGlb44A or
// beyond, past R: streamed bodies to the end of the step
__device__ __forceinline__ int glb44_mode(const Glb44Stream &st, const int b, const int n, const bool deep)
{
  return deep ? kGlb44Glb : (b + n - 1 + kGlb44AL < st.R) ? kGlb44Lds : kGlb44Seam;
}
// behind a seam body: its fetches have landed
__device__ __forceinline__ void glb44_land(m44_f4 (&w)[kGlb44A])
{
#pragma unroll
  for (int i = 0; i < kGlb44A; i++) asm volatile("" : "+v"(w[i]));
}
// the ring turned left by r quads (wave-uniform, 0 <= r < kGlb44A <= 16): w[0] is the next quad again
template <int S>
__device__ __forceinline__ void glb44_rotate(m44_f4 (&w)[kGlb44A])
{
  m44_f4 x[kGlb44A];
#pragma unroll
  for (int i = 0; i < kGlb44A; i++) x[i] = w[(i + S) % kGlb44A];
#pragma unroll
  for (int i = 0; i < kGlb44A; i++) w[i] = x[i];
}
__device__ __forceinline__ void glb44_turn(m44_f4 (&w)[kGlb44A], const int r)
{
  if (r & 1) glb44_rotate<1>(w);
  if constexpr (kGlb44A > 2) {
    if (r & 2) glb44_rotate<2>(w);
  }
  if constexpr (kGlb44A > 4) {
    if (r & 4) glb44_rotate<4 % kGlb44A>(w);
  }
  if constexpr (kGlb44A > 8) {
    if (r & 8) glb44_rotate<8 % kGlb44A>(w);
  }
}

// one input set of a layer of H halves: stream quads b + Q H + h are quad Q (k-steps 4 Q .. 4 Q + 3 of the set) of d[h] -- the
// same A operand, the k-steps of the H independent chains alternate.  w: the ring, quad b + i in w[i % kGlb44A]
template <int H, int MODE, int Q>
__device__ __forceinline__ void glb44_body(m44_f4 (&d)[4], const float (&Ts)[4], m44_f4 (&w)[kGlb44A], const Glb44Stream &st, const int b,
                                           const int nq)
{
  if constexpr (Q < 16) {
    if (Q > 0 && Q >= nq) return;  // wave-uniform
    if constexpr (MODE == kGlb44Seam && Q == 0) {  // the ring from kGlb44AL to kGlb44A quads
#pragma unroll
      for (int i = kGlb44AL; i < kGlb44A; i++) w[i] = glb44_fetch<kGlb44Seam>(st, b + i);
    }
    m44_f4 x[H];
#pragma unroll
    for (int h = 0; h < H; h++) {
      x[h] = w[(Q * H + h) % kGlb44A];
      if constexpr (MODE == kGlb44Lds) w[(Q * H + h + kGlb44AL) % kGlb44A] = glb44_fetch<kGlb44Lds>(st, b + Q * H + h + kGlb44AL);
      else w[(Q * H + h) % kGlb44A] = glb44_fetch<MODE>(st, b + Q * H + h + kGlb44A);
    }
    lds_pin_reads();
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
      for (int h = 0; h < H; h++) d[h] = __builtin_amdgcn_mfma_f32_4x4x1f32(Ts[i], x[h][i], d[h], 4, Q, 0);
    }
    glb44_body<H, MODE, Q + 1>(d, Ts, w, st, b, nq);
  }
}
template <int H>
__device__ __forceinline__ void glb44_set(m44_f4 (&d)[4], const float (&Ts)[4], m44_f4 (&w)[kGlb44A], const Glb44Stream &st, int &b, bool &deep,
                                          const int nq)
{
  const int n = nq * H;
  const int mode = glb44_mode(st, b, n, deep);  // wave-uniform
  if (mode == kGlb44Lds) glb44_body<H, kGlb44Lds, 0>(d, Ts, w, st, b, nq);
  else if (mode == kGlb44Glb) glb44_body<H, kGlb44Glb, 0>(d, Ts, w, st, b, nq);
  else {
    glb44_body<H, kGlb44Seam, 0>(d, Ts, w, st, b, nq);
    glb44_land(w);
    deep = true;
  }
  b += n;
  glb44_turn(w, n % kGlb44A);
}

// layer 0 (6 inputs, two quads per half, in registers): [s3, s4, s5, s6, u0, u1] -- row c of the state register is component c: ABID = 4 c
template <int H>
__device__ __forceinline__ void glb44_layer0(m44_f4 (&d)[4], const float sv, const f32x2 u, const m44_f4 (&w0)[4][2])
{
#pragma unroll
  for (int c = 0; c < 4; c++) {
#pragma unroll
    for (int h = 0; h < H; h++) {
      switch (c) {  // ABID is an immediate
        case 0: d[h] = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0[h][0][0], d[h], 4, 0, 0); break;
        case 1: d[h] = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0[h][0][1], d[h], 4, 4, 0); break;
        case 2: d[h] = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0[h][0][2], d[h], 4, 8, 0); break;
        default: d[h] = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0[h][0][3], d[h], 4, 12, 0); break;
      }
    }
  }
#pragma unroll
  for (int h = 0; h < H; h++) d[h] = __builtin_amdgcn_mfma_f32_4x4x1f32(u.x, w0[h][1][0], d[h], 4, 0, 0);
#pragma unroll
  for (int h = 0; h < H; h++) d[h] = __builtin_amdgcn_mfma_f32_4x4x1f32(u.y, w0[h][1][1], d[h], 4, 0, 0);
}

template <bool GATED>
__device__ __forceinline__ void glb44_dynamics(const RolloutArgs &a, const M44LayerList &net, M44GroupShared &sh, const m44_f4 *img, const int R_arg,
                                               const int w)
{
  const int lane = threadIdx.x & 63;
  const bool hi = (lane & 2) != 0, od = (lane & 1) != 0;
  const int T = a.T;
  const int n_w = __builtin_amdgcn_readfirstlane(net.n_layers) - 1;  // weight layers; the last one is the output layer
  const m44_f4 *pk = img + lane;                                      // bias quad j: pk[j * 64]
  // per weight layer j, bits 9 j .. 9 j + 6: its quads (1..64), bits 9 j + 7, 8: its halves - 1 -- the T loop reads no kernel argument
  unsigned long long lay_all = 0;
#pragma unroll
  for (int j = 0; j < 7; j++)
    lay_all |= (unsigned long long)(glb44_quads_of(j == 0 ? kNetIn : net.layers[j]) | ((j + 1 < n_w ? glb44_halves_of(net.layers[j + 1]) - 1 : 0) << 7)) << (9 * j);
  const int H0 = (((int)lay_all >> 7) & 3) + 1;
  const m44_f4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  // layer 0, its bias quad and the output layer's bias stay in registers
  const m44_f4 *const pw0 = pk + kGlb44BiasQuads * 64;
  m44_f4 w0[4][2];
#pragma unroll
  for (int h = 0; h < 4; h++) {
    w0[h][0] = h < H0 ? pw0[h * 64] : zero4;
    w0[h][1] = h < H0 ? pw0[(H0 + h) * 64] : zero4;
  }
  const m44_f4 bq0 = pk[0];
  const float bo = pk[(n_w - 1) * 64][0];
  // a lane beyond the first hidden layer's width holds no neuron (rollout_lds128.hip: pad0)
  bool pad[4];
#pragma unroll
  for (int h = 0; h < 4; h++) pad[h] = lane + 64 * h >= net.layers[1];
  const int head_f4 = (kGlb44BiasQuads + 2 * H0) * 64;
  const Glb44Stream st = {(Glb44LdsPtr)(pk + head_f4), (Glb44GlbPtr)(reinterpret_cast<const m44_f4 *>(a.wpack) + head_f4 + lane),
                          __builtin_amdgcn_readfirstlane(R_arg)};

  float act[4][4], Tr[4][4];
#pragma unroll
  for (int h = 0; h < 4; h++)
#pragma unroll
    for (int i = 0; i < 4; i++) act[h][i] = Tr[h][i] = 0.0f;

  m44_f4 wq[kGlb44A];
#pragma unroll
  for (int i = 0; i < kGlb44A; i++) wq[i] = zero4;

  M44Wave<GATED> wv(a, sh, w);
  for (int t = 0; t < T - 1; t++) {
    const f32x2 u = wv.open(t);
    const float sv = wv.sv;
    // the first quads of the stream, requested in front of layer 0; deep: the ring holds kGlb44A quads, not kGlb44AL
    bool deep = st.R < kGlb44AL;  // wave-uniform
    if (!deep) {
#pragma unroll
      for (int i = 0; i < kGlb44AL; i++) wq[i] = glb44_fetch<kGlb44Lds>(st, i);
    } else if (st.R == 0) {
#pragma unroll
      for (int i = 0; i < kGlb44A; i++) wq[i] = glb44_fetch<kGlb44Glb>(st, i);
    } else {
#pragma unroll
      for (int i = 0; i < kGlb44A; i++) wq[i] = glb44_fetch<kGlb44Seam>(st, i);
      glb44_land(wq);
    }
    lds_pin_reads();
    m44_f4 d[4] = {zero4, zero4, zero4, zero4};
    int H = H0;  // the halves of the layer whose D is at hand
    if (H == 1) glb44_layer0<1>(d, sv, u, w0);
    else if (H == 2) glb44_layer0<2>(d, sv, u, w0);
    else if (H == 3) glb44_layer0<3>(d, sv, u, w0);
    else glb44_layer0<4>(d, sv, u, w0);
    wv.request(t + 1);
#pragma unroll
    for (int h = 0; h < 4; h++) {
      if (h > 0 && h >= H) break;  // wave-uniform
      m44_tanh(d[h], bq0[h], act[h]);
      if (pad[h]) act[h][0] = act[h][1] = act[h][2] = act[h][3] = 0.0f;
    }
    int b = 0;
    for (int j = 1;; j++) {
      const int lay = (int)(lay_all >> (9 * j));
      const int nq = lay & 127, Hn = ((lay >> 7) & 3) + 1;  // the output layer: one accumulator
      const m44_f4 bq = pk[j * 64];                         // arrives under the chains
#pragma unroll
      for (int h = 0; h < 4; h++) {
        if (h > 0 && h >= H) break;  // wave-uniform
        m44_transpose(act[h], Tr[h], hi, od);
      }
#pragma unroll
      for (int h = 0; h < 4; h++) d[h] = zero4;
      for (int s = 0; 16 * s < nq; s++) {
        const int nqs = nq - 16 * s < 16 ? nq - 16 * s : 16;
        float Ts[4];
#pragma unroll
        for (int i = 0; i < 4; i++) Ts[i] = s == 0 ? Tr[0][i] : s == 1 ? Tr[1][i] : s == 2 ? Tr[2][i] : Tr[3][i];  // wave-uniform
        if (Hn == 1) glb44_set<1>(d, Ts, wq, st, b, deep, nqs);
        else if (Hn == 2) glb44_set<2>(d, Ts, wq, st, b, deep, nqs);
        else if (Hn == 3) glb44_set<3>(d, Ts, wq, st, b, deep, nqs);
        else glb44_set<4>(d, Ts, wq, st, b, deep, nqs);
      }
      if (j == n_w - 1) break;
      H = Hn;
#pragma unroll
      for (int h = 0; h < 4; h++) {
        if (h > 0 && h >= H) break;  // wave-uniform
        m44_tanh(d[h], bq[h], act[h]);
      }
    }
    // the output layer's D: lane 16 c of register r = output c of rollout r; transposed: quad 0 of row c, register 0
    float o[4] = {d[0][0], d[0][1], d[0][2], d[0][3]}, oT[4];
    m44_transpose(o, oT, hi, od);
    wv.close(t, a.dt, oT[0] + bo);
  }
  wv.finish(T - 1, sh, w);
}

// m44_group.hpp's FORM: the head and the first R quads of the stream behind the shared state, copied by all threads
struct Glb44Form {
  using Shared = M44GroupShared;
  const M44LayerList &net;
  const int R;
  __device__ __forceinline__ m44_f4 *image() const { return reinterpret_cast<m44_f4 *>(m44_group_smem + kM44GroupImageOffset); }
  __device__ __forceinline__ void stage_by_all(const RolloutArgs &a, Shared &) const
  {
    m44_f4 *img = image();
    const m44_f4 *src = reinterpret_cast<const m44_f4 *>(a.wpack);
    const int n = (kGlb44BiasQuads + 2 * glb44_halves_of(net.layers[1]) + R) * 64;
    for (int q = threadIdx.x; q < n; q += 512) img[q] = src[q];
  }
  __device__ __forceinline__ void stage_by_wave1(const RolloutArgs &, Shared &) const {}
  template <bool GATED>
  __device__ __forceinline__ void dynamics(const RolloutArgs &a, Shared &sh, const int w) const
  {
    glb44_dynamics<GATED>(a, net, sh, image(), R, w);
  }
};

// R: the resident stream quads, what the launcher sized the dynamic LDS for
template <bool AFFINE, bool CTRL, bool GATED>
__global__ __launch_bounds__(512) void rollout_glb44_kernel(const RolloutArgs a, const M44LayerList net, const int R)
{
  m44_group_body<AFFINE, CTRL, GATED>(a, *reinterpret_cast<M44GroupShared *>(m44_group_smem), Glb44Form{net, R});
}
// all instances have the SAME layer list and the same R; each copies its own image from its own a.wpack
template <bool AFFINE, bool CTRL, bool GATED, int NB>
__global__ __launch_bounds__(512) void rollout_glb44_batch_kernel(const QuadBatchArgsT<NB> b, const M44LayerList net, const int R)
{
  m44_group_batch_body<AFFINE, CTRL, GATED, NB>(b, *reinterpret_cast<M44GroupShared *>(m44_group_smem), Glb44Form{net, R});
}

hipError_t launch_rollout_glb44(const NetDesc &net, const RolloutArgs &a, int cap, hipStream_t stream)
{
  if (!glb44_supported(net) || a.K % kRolloutsPerWave != 0) return hipErrorInvalidValue;
  const dim3 grid(a.K / kRolloutsPerWave), block(512);
  const int R = glb44_resident_quads(net, cap);
  const size_t lds = glb44_lds_bytes(net, cap);
  if (lds > kGlb44MaxBytes) return hipErrorInvalidValue;
  const M44LayerList nd = m44_layer_list_of(net);
  return dispatch_rollout_flags(a.cost.affine != 0, a.cost.need_control_cost != 0, a.gate != nullptr, [&](auto af, auto ct, auto ga) {
    constexpr auto kern = &rollout_glb44_kernel<decltype(af)::value, decltype(ct)::value, decltype(ga)::value>;
    if (hipError_t e = raise_lds_limit_once<kern>(kGlb44MaxBytes); e != hipSuccess) return e;
    MPPI_LAUNCH_ROLLOUT(kern, grid, block, lds, stream, a, nd, R);
    return hipGetLastError();
  });
}

// two instances of ONE layer list (net) and one cap in one launch
hipError_t launch_rollout_glb44_batch(const NetDesc &net, const QuadBatchArgs &b, int cap, hipStream_t stream)
{
  BatchFlags f;
  if (b.n != 2 || !glb44_supported(net) || !batch_flags_of(b, f)) return hipErrorInvalidValue;
  const QuadBatchArgsT<2> b2 = batch_args_prefix<2>(b);
  const dim3 grid(f.gmax, 2), block(512);
  const int R = glb44_resident_quads(net, cap);
  const size_t lds = glb44_lds_bytes(net, cap);
  if (lds > kGlb44MaxBytes) return hipErrorInvalidValue;
  const M44LayerList nd = m44_layer_list_of(net);
  return dispatch_rollout_flags(f.affine, f.ctrl, f.gated, [&](auto af, auto ct, auto ga) {
    constexpr auto kern = &rollout_glb44_batch_kernel<decltype(af)::value, decltype(ct)::value, decltype(ga)::value, 2>;
    if (hipError_t e = raise_lds_limit_once<kern>(kGlb44MaxBytes); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, lds, stream, b2, nd, R);
    return hipGetLastError();
  });
}

}  // namespace mppi
