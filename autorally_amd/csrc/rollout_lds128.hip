// rollout_lds128.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) for gfx950, the latency form of ANY layer list with
// hidden widths up to 128 (rollout_lds44.hip stops at 64): v_mfma_f32_4x4x1 with A-matrix broadcast, the B operand read
// from LDS, the layer list a kernel ARGUMENT -- rollout_lds44.hip's group, riders, rings and barrier, with
//   * a hidden layer of nout outputs as H = ceil(nout / 64) "halves": half h holds neurons 64 h .. 64 h + 63 in its own
//     accumulator d[h] (a lane is neuron 64 h + lane).  A layer of one half never enters the code of the second one;
//   * a layer's up to 128 inputs as two transposed activation sets: k steps 0..63 (quads 0..15) take their A operand from
//     T0[k & 3], ABID = k >> 2, k steps 64..127 (quads 16..31) from T1[k & 3], ABID = (k - 64) >> 2.  Every accumulator sees
//     k = 0, 1, .. nin - 1 ascending, one instruction per step: the fmaf chain of neural_net_model.cu:379-394, so the form
//     is bit-identical to "valu_lds" (and to "lds44" on lists that are 64 wide at the most);
//   * the steps of the two halves interleaved in the instruction stream, quad by quad: two independent chains per wave;
//   * wave-uniform exits: every 4 steps at ceil(nin / 4), and the whole second half when nout <= 64.  A padded k step adds
//     fma(0, 0, d) = d (the accumulator starts at +0 and never is -0), a padded neuron is tanh(0 + 0) = 0;
//   * the OUTPUT layer as one more chain of up to 32 quads into ONE accumulator: W_out[c][k] sits at lane 16 c of the B image
//     (zeros elsewhere), so after the transpose quad 0 of row c holds output c of rollouts 0..3 in register 0 -- the layout
//     of the state register.
// Image (pack_lds128_weights, abi_pack.hip): float4 q of lane l at float4 index q * 64 + l.
//   q 0 .. kLds128BiasQuads-1  float e = 2 j + h of lane l: bias of neuron 64 h + l of weight layer j -- hidden layers:
//                              b x kTanhScale (0 where the neuron does not exist); output layer (e = 2 j): b_out[l >> 4]
//   then per weight layer ceil(nin / 4) x H quads (H = 1 for the output layer), INTERLEAVED: quad q' H + h of the layer is
//                              (W[64 h + l][4 q'], .. W[64 h + l][4 q' + 3]); the output layer's row c at lane 16 c
//   then kLds44Ahead quads of zeros (the read-ahead of the last layer stays inside the image)
// The interleaved order makes a layer's B operands ONE stream in the order of their use: the read-ahead is kLds44Ahead
// stream elements whatever H is.
#include "m44_group.hpp"

namespace mppi {

constexpr size_t kLds128MaxBytes = 160 * 1024;  // the dynamic-LDS limit the launcher requests

__host__ __device__ inline int lds128_quads_of(int nin) { return (nin + 3) >> 2; }
__host__ __device__ inline int lds128_halves_of(int nout) { return nout > 64 ? 2 : 1; }

// one half per layer (and the output layer): stream element Q is quad Q of the ONE accumulator; quads 16.. read T1
template <int Q>
__device__ __forceinline__ void lds128_chain1(m44_f4 &d, const float (&T0)[4], const float (&T1)[4], m44_f4 (&w)[kLds44Ahead],
                                              const m44_f4 *p, const int nq)
{
  if constexpr (Q < 32) {
    if (Q > 0 && Q >= nq) return;  // wave-uniform
    const m44_f4 x = w[Q % kLds44Ahead];
    if constexpr (Q + kLds44Ahead < 32) w[Q % kLds44Ahead] = p[(Q + kLds44Ahead) * 64];
    lds_pin_reads();
    const float (&T)[4] = Q < 16 ? T0 : T1;
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(T[0], x[0], d, 4, Q & 15, 0);
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(T[1], x[1], d, 4, Q & 15, 0);
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(T[2], x[2], d, 4, Q & 15, 0);
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(T[3], x[3], d, 4, Q & 15, 0);
    lds128_chain1<Q + 1>(d, T0, T1, w, p, nq);
  }
}

// two halves: stream elements 2 Q and 2 Q + 1 are quad Q of d0 and of d1 -- the same A operand, the k steps of the two
// independent chains alternate in the instruction stream
template <int Q>
__device__ __forceinline__ void lds128_chain2(m44_f4 &d0, m44_f4 &d1, const float (&T0)[4], const float (&T1)[4],
                                              m44_f4 (&w)[kLds44Ahead], const m44_f4 *p, const int nq)
{
  if constexpr (Q < 32) {
    if (Q > 0 && Q >= nq) return;  // wave-uniform
    constexpr int S = 2 * Q;
    const m44_f4 x0 = w[S % kLds44Ahead];
    if constexpr (S + kLds44Ahead < 64) w[S % kLds44Ahead] = p[(S + kLds44Ahead) * 64];
    const m44_f4 x1 = w[(S + 1) % kLds44Ahead];
    if constexpr (S + 1 + kLds44Ahead < 64) w[(S + 1) % kLds44Ahead] = p[(S + 1 + kLds44Ahead) * 64];
    lds_pin_reads();
    const float (&T)[4] = Q < 16 ? T0 : T1;
    d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(T[0], x0[0], d0, 4, Q & 15, 0);
    d1 = __builtin_amdgcn_mfma_f32_4x4x1f32(T[0], x1[0], d1, 4, Q & 15, 0);
    d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(T[1], x0[1], d0, 4, Q & 15, 0);
    d1 = __builtin_amdgcn_mfma_f32_4x4x1f32(T[1], x1[1], d1, 4, Q & 15, 0);
    d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(T[2], x0[2], d0, 4, Q & 15, 0);
    d1 = __builtin_amdgcn_mfma_f32_4x4x1f32(T[2], x1[2], d1, 4, Q & 15, 0);
    d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(T[3], x0[3], d0, 4, Q & 15, 0);
    d1 = __builtin_amdgcn_mfma_f32_4x4x1f32(T[3], x1[3], d1, 4, Q & 15, 0);
    lds128_chain2<Q + 1>(d0, d1, T0, T1, w, p, nq);
  }
}

template <bool GATED>
__device__ __forceinline__ void lds128_dynamics(const RolloutArgs &a, const M44LayerList &net, M44GroupShared &sh, const m44_f4 *img, const int w)
{
  const int lane = threadIdx.x & 63;
  const bool hi = (lane & 2) != 0, od = (lane & 1) != 0;
  const int T = a.T;
  const int n_w = net.n_layers - 1;  // weight layers; the last one is the output layer
  const m44_f4 *pk = img + lane;
  const float *pb = reinterpret_cast<const float *>(pk);  // bias e = 2 j + h: pb[(e >> 2) * 256 + (e & 3)]
  // per weight layer j, bits 8 j .. 8 j + 5: its quads, bit 8 j + 6: it has a second half -- the T loop reads no kernel argument
  unsigned long long lay_all = 0;
#pragma unroll
  for (int j = 0; j < 7; j++)
    lay_all |= (unsigned long long)(lds128_quads_of(j == 0 ? kNetIn : net.layers[j]) | ((j + 1 < n_w && net.layers[j + 1] > 64) ? 64 : 0)) << (8 * j);
  // layer 0 (6 inputs, two quads per half) and the first and the last bias stay in registers
  const bool two0 = ((int)(lay_all >> 6) & 1) != 0;
  const m44_f4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  const m44_f4 *const pw0 = pk + kLds128BiasQuads * 64;
  const m44_f4 w0a = pw0[0], w0b = two0 ? pw0[2 * 64] : pw0[64];
  const m44_f4 w0c = two0 ? pw0[64] : zero4, w0d = two0 ? pw0[3 * 64] : zero4;  // the second half's two quads
  const float bs0 = pb[0], bs0h = pb[1];
  // a lane beyond the first hidden layer's width holds no neuron: its zero weights times an infinite state entry are NaN, which
  // the next layer's padded k steps (zero weights again) would spread to every neuron; the reference multiplies real weights only
  const bool pad0 = lane >= net.layers[1], pad0h = lane + 64 >= net.layers[1];
  const float bo = pb[((n_w - 1) >> 1) * 256 + (((n_w - 1) & 1) << 1)];
  const m44_f4 *const p1 = pw0 + (two0 ? 4 : 2) * 64;  // layer 1

  M44Wave<GATED> wv(a, sh, w);
  for (int t = 0; t < T - 1; t++) {
    const f32x2 u = wv.open(t);
    const float sv = wv.sv;
    // the first stream elements of layer 1, requested in front of layer 0
    m44_f4 wq[kLds44Ahead];
#pragma unroll
    for (int q = 0; q < kLds44Ahead; q++) wq[q] = p1[q * 64];
    // layer 0: [s3, s4, s5, s6, u0, u1] -- row c of the state register is component c: ABID = 4 c
    m44_f4 d0 = zero4, d1 = zero4;
    float act0[4], act1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, T0[4], T1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool two = two0;  // the layer whose D is at hand has a second half
    if (two) {
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0a[0], d0, 4, 0, 0);
      d1 = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0c[0], d1, 4, 0, 0);
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0a[1], d0, 4, 4, 0);
      d1 = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0c[1], d1, 4, 4, 0);
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0a[2], d0, 4, 8, 0);
      d1 = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0c[2], d1, 4, 8, 0);
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0a[3], d0, 4, 12, 0);
      d1 = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0c[3], d1, 4, 12, 0);
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(u.x, w0b[0], d0, 4, 0, 0);
      d1 = __builtin_amdgcn_mfma_f32_4x4x1f32(u.x, w0d[0], d1, 4, 0, 0);
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(u.y, w0b[1], d0, 4, 0, 0);
      d1 = __builtin_amdgcn_mfma_f32_4x4x1f32(u.y, w0d[1], d1, 4, 0, 0);
    } else {
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0a[0], d0, 4, 0, 0);
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0a[1], d0, 4, 4, 0);
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0a[2], d0, 4, 8, 0);
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0a[3], d0, 4, 12, 0);
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(u.x, w0b[0], d0, 4, 0, 0);
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(u.y, w0b[1], d0, 4, 0, 0);
    }
    wv.request(t + 1);
    m44_tanh(d0, bs0, act0);
    if (pad0) act0[0] = act0[1] = act0[2] = act0[3] = 0.0f;
    if (two) {
      m44_tanh(d1, bs0h, act1);
      if (pad0h) act1[0] = act1[1] = act1[2] = act1[3] = 0.0f;
    }
    const m44_f4 *p = p1;
    for (int j = 1;; j++) {
      const int lay = (int)(lay_all >> (8 * j));
      const int nq = lay & 63;
      m44_transpose(act0, T0, hi, od);
      if (two) m44_transpose(act1, T1, hi, od);
      d0 = zero4;
      two = (lay & 64) != 0;  // never the output layer: one accumulator
      if (two) {
        d1 = zero4;
        lds128_chain2<0>(d0, d1, T0, T1, wq, p, nq);
        p += 2 * nq * 64;
      } else {
        lds128_chain1<0>(d0, T0, T1, wq, p, nq);
        p += nq * 64;
      }
      if (j == n_w - 1) break;
      const float bs =pb[(j >> 1) * 256 + ((j & 1) << 1)], bsh = pb[(j >> 1) * 256 + ((j & 1) << 1) + 1];
#pragma unroll
      for (int q = 0; q < kLds44Ahead; q++) wq[q] = p[q * 64];  // the next layer's first elements arrive under the tanh
      m44_tanh(d0, bs, act0);
      if (two) m44_tanh(d1, bsh, act1);
    }
    // the output layer's D: lane 16 c of register r = output c of rollout r; transposed: quad 0 of row c, register 0
    act0[0] = d0[0]; act0[1] = d0[1]; act0[2] = d0[2]; act0[3] = d0[3];
    m44_transpose(act0, T0, hi, od);
    wv.close(t, a.dt, T0[0] + bo);
  }
  wv.finish(T - 1, sh, w);
}

// the kernels: m44_group.hpp's group with the image behind the shared state as the group's dynamic LDS
template <bool AFFINE, bool CTRL, bool GATED>
__global__ __launch_bounds__(512) void rollout_lds128_kernel(const RolloutArgs a, const M44LayerList net, const int img_f4)
{
  m44_lds_kernel_body<&lds128_dynamics<GATED>, AFFINE, CTRL, GATED>(a, net, img_f4);
}
template <bool AFFINE, bool CTRL, bool GATED, int NB>
__global__ __launch_bounds__(512) void rollout_lds128_batch_kernel(const QuadBatchArgsT<NB> b, const M44LayerList net, const int img_f4)
{
  m44_lds_batch_kernel_body<&lds128_dynamics<GATED>, AFFINE, CTRL, GATED, NB>(b, net, img_f4);
}

int lds128_pack_floats(const NetDesc &net)
{
  int q = kLds128BiasQuads + kLds44Ahead;
  const int n_w = net.n_layers - 1;
  for (int j = 0; j < n_w; j++) q += lds128_quads_of(net.layers[j]) * (j + 1 < n_w ? lds128_halves_of(net.layers[j + 1]) : 1);
  return q * 64 * 4;
}

// the group's dynamic LDS: shared state + image; 0 for a list the form does not take whatever its size
size_t lds128_lds_bytes(const NetDesc &net)
{
  if (!lds_list_ok(net, 128)) return 0;
  return kM44GroupImageOffset + sizeof(float) * (size_t)lds128_pack_floats(net);
}
size_t lds128_lds_limit() { return kLds128MaxBytes; }

// every list 6 -> hidden widths 1..128 -> 4 with at least one hidden layer whose image fits one workgroup's LDS
bool lds128_supported(const NetDesc &net) { return lds_list_ok(net, 128) && lds128_lds_bytes(net) <= kLds128MaxBytes; }

hipError_t launch_rollout_lds128(const NetDesc &net, const RolloutArgs &a, hipStream_t stream)
{
  if (!lds128_supported(net) || a.K % kRolloutsPerWave != 0) return hipErrorInvalidValue;
  const dim3 grid(a.K / kRolloutsPerWave), block(512);
  const int img_f4 = lds128_pack_floats(net) / 4;
  const size_t lds = lds128_lds_bytes(net);
  const M44LayerList nd = m44_layer_list_of(net);
  return dispatch_rollout_flags(a.cost.affine != 0, a.cost.need_control_cost != 0, a.gate != nullptr, [&](auto af, auto ct, auto ga) {
    constexpr auto kern = &rollout_lds128_kernel<decltype(af)::value, decltype(ct)::value, decltype(ga)::value>;
    if (hipError_t e = raise_lds_limit_once<kern>(kLds128MaxBytes); e != hipSuccess) return e;
    MPPI_LAUNCH_ROLLOUT(kern, grid, block, lds, stream, a, nd, img_f4);
    return hipGetLastError();
  });
}

// two instances of ONE layer list (net) in one launch
hipError_t launch_rollout_lds128_batch(const NetDesc &net, const QuadBatchArgs &b, hipStream_t stream)
{
  BatchFlags f;
  if (b.n != 2 || !lds128_supported(net) || !batch_flags_of(b, f)) return hipErrorInvalidValue;
  const QuadBatchArgsT<2> b2 = batch_args_prefix<2>(b);
  const dim3 grid(f.gmax, 2), block(512);
  const int img_f4 = lds128_pack_floats(net) / 4;
  const size_t lds = lds128_lds_bytes(net);
  const M44LayerList nd = m44_layer_list_of(net);
  return dispatch_rollout_flags(f.affine, f.ctrl, f.gated, [&](auto af, auto ct, auto ga) {
    constexpr auto kern = &rollout_lds128_batch_kernel<decltype(af)::value, decltype(ct)::value, decltype(ga)::value, 2>;
    if (hipError_t e = raise_lds_limit_once<kern>(kLds128MaxBytes); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, lds, stream, b2, nd, img_f4);
    return hipGetLastError();
  });
}

}  // namespace mppi
