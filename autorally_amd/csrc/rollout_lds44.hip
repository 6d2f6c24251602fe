// rollout_lds44.hip -- rolloutKernel (PI/mppi_controller.cu:72-184) for gfx950, the latency form of ANY layer list with
// hidden widths up to 64 (the reference's scripts/ml_pipeline trains any nn_layers; rollout_m44.hip serves two shapes):
// v_mfma_f32_4x4x1 with A-matrix broadcast as in rollout_m44.hip -- a lane is a neuron, one instruction is step k of the
// k-ascending fmaf chain of neural_net_model.cu:379-394 for 4 rollouts x 64 neurons -- with the B operand (lane n: W[n][k])
// read from LDS instead of held in registers, so that the layer list is a kernel ARGUMENT and the kernel has no network
// template parameter.
//   * the group is rollout_m44.hip's: 512 threads per 16 rollouts, 4 dynamics waves x 4 rollouts + the four riders of
//     group_roles.hpp, record rings in LDS, one barrier;
//   * the weights of ALL layers sit in LDS (pack_lds44_weights, abi_pack.hip): per layer ceil(nin / 4) float4 per lane,
//     k and n padded with zeros.  A padded k step adds fma(0, 0, d) = d (the accumulator starts at +0 and never is -0),
//     a padded neuron is tanh(0 + 0) = 0;
//   * a layer is ONE chain, k ascending; the block index is an immediate, so the 64 steps are unrolled with a wave-uniform
//     exit every 4 steps; the next kLds44Ahead quads of weights are in flight (ds_read_b128: 4 k steps per read);
//   * the OUTPUT layer is one more chain: W_out[c][k] sits at lane 16 c of the B image (zeros elsewhere), so after the
//     transpose quad 0 of row c holds output c of rollouts 0..3 in register 0 -- the layout of the state register.  The
//     reference's order in EVERY layer: bit-identical to "valu_lds", "valu", "quad", "row_exact".
#include "m44_group.hpp"

namespace mppi {

// Image (pack_lds44_weights): float4 q of lane l at float4 index q * 64 + l.
//   q 0 .. kLds44BiasQuads-1   float e = 4 q + c: bias of layer e for lane l -- hidden layers: b[l] x kTanhScale (0 for l >= nout);
//                              output layer: b_out[l >> 4]
//   then per layer ceil(nin / 4) quads: (W[l][4 q'], .. W[l][4 q' + 3]); output layer: row c at lane 16 c
//   then kLds44Ahead quads of zeros (the read-ahead of the last layer stays inside the image)
__host__ __device__ inline int lds44_quads_of(int nin) { return (nin + 3) >> 2; }

template <int Q>
__device__ __forceinline__ void lds44_chain(m44_f4 &d, const float (&T)[4], m44_f4 (&w)[kLds44Ahead], const m44_f4 *p, const int nq)
{
  if constexpr (Q < 16) {
    if (Q > 0 && Q >= nq) return;  // wave-uniform
    const m44_f4 x = w[Q % kLds44Ahead];
    if constexpr (Q + kLds44Ahead < 16) w[Q % kLds44Ahead] = p[(Q + kLds44Ahead) * 64];
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(T[0], x[0], d, 4, Q, 0);
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(T[1], x[1], d, 4, Q, 0);
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(T[2], x[2], d, 4, Q, 0);
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(T[3], x[3], d, 4, Q, 0);
    lds44_chain<Q + 1>(d, T, w, p, nq);
  }
}

template <bool GATED>
__device__ __forceinline__ void lds44_dynamics(const RolloutArgs &a, const M44LayerList &net, M44GroupShared &sh, const m44_f4 *img, const int w)
{
  const int lane = threadIdx.x & 63;
  const bool hi = (lane & 2) != 0, od = (lane & 1) != 0;
  const int T = a.T;
  const int n_w = net.n_layers - 1;  // weight layers; the last one is the output layer
  const m44_f4 *pk = img + lane;
  const float *pb = reinterpret_cast<const float *>(pk);  // bias of layer e: pb[(e >> 2) * 256 + (e & 3)]
  // layer 0 (6 inputs, two quads) and the first and the last bias stay in registers
  const m44_f4 w0a = pk[kLds44BiasQuads * 64], w0b = pk[(kLds44BiasQuads + 1) * 64];
  const float bs0 = pb[0];
  // a lane beyond the first hidden layer's width holds no neuron: its zero weights times an infinite state entry are NaN, which
  // the next layer's padded k steps (zero weights again) would spread to every neuron; the reference multiplies real weights only
  const bool pad0 = lane >= net.layers[1];
  const float bo = pb[((n_w - 1) >> 2) * 256 + ((n_w - 1) & 3)];
  const m44_f4 *const p1 = pk + (kLds44BiasQuads + 2) * 64;  // layer 1
  // quads of layer l in bits 5 l .. 5 l + 4 of a scalar: the T loop reads no kernel argument
  unsigned long long nq_all = 0;
#pragma unroll
  for (int l = 1; l < 8; l++) nq_all |= (unsigned long long)lds44_quads_of(net.layers[l]) << (5 * l);

  M44Wave<GATED> wv(a, sh, w);
  for (int t = 0; t < T - 1; t++) {
    const f32x2 u = wv.open(t);
    const float sv = wv.sv;
    // the first quads of layer 1, requested in front of layer 0
    m44_f4 wq[kLds44Ahead];
#pragma unroll
    for (int q = 0; q < kLds44Ahead; q++) wq[q] = p1[q * 64];
    // layer 0: [s3, s4, s5, s6, u0, u1] -- row c of the state register is component c: ABID = 4 c
    m44_f4 d = {0.0f, 0.0f, 0.0f, 0.0f};
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0a[0], d, 4, 0, 0);
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0a[1], d, 4, 4, 0);
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0a[2], d, 4, 8, 0);
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(sv, w0a[3], d, 4, 12, 0);
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(u.x, w0b[0], d, 4, 0, 0);
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(u.y, w0b[1], d, 4, 0, 0);
    wv.request(t + 1);
    float act[4], Tr[4];
    m44_tanh(d, bs0, act);
    if (pad0) act[0] = act[1] = act[2] = act[3] = 0.0f;
    const m44_f4 *p = p1;
    for (int l = 1;; l++) {
      const int nq = (int)(nq_all >> (5 * l)) & 31;
      m44_transpose(act, Tr, hi, od);
      d = m44_f4{0.0f, 0.0f, 0.0f, 0.0f};
      lds44_chain<0>(d, Tr, wq, p, nq);
      if (l == n_w - 1) break;
      p += nq * 64;
      const float bs = pb[(l >> 2) * 256 + (l & 3)];
#pragma unroll
      for (int q = 0; q < kLds44Ahead; q++) wq[q] = p[q * 64];  // the next layer's first quads arrive under the tanh
      m44_tanh(d, bs, act);
    }
    // the output layer's D: lane 16 c of register r = output c of rollout r; transposed: quad 0 of row c, register 0
    act[0] = d[0]; act[1] = d[1]; act[2] = d[2]; act[3] = d[3];
    m44_transpose(act, Tr, hi, od);
    wv.close(t, a.dt, Tr[0] + bo);
  }
  wv.finish(T - 1, sh, w);
}

// the kernels: m44_group.hpp's group with the image behind the shared state as the group's dynamic LDS
template <bool AFFINE, bool CTRL, bool GATED>
__global__ __launch_bounds__(512) void rollout_lds44_kernel(const RolloutArgs a, const M44LayerList net, const int img_f4)
{
  m44_lds_kernel_body<&lds44_dynamics<GATED>, AFFINE, CTRL, GATED>(a, net, img_f4);
}
template <bool AFFINE, bool CTRL, bool GATED, int NB>
__global__ __launch_bounds__(512) void rollout_lds44_batch_kernel(const QuadBatchArgsT<NB> b, const M44LayerList net, const int img_f4)
{
  m44_lds_batch_kernel_body<&lds44_dynamics<GATED>, AFFINE, CTRL, GATED, NB>(b, net, img_f4);
}

// every list 6 -> hidden widths 1..64 -> 4 with at least one hidden layer
bool lds44_supported(const NetDesc &net) { return lds_list_ok(net, 64); }

int lds44_pack_floats(const NetDesc &net)
{
  int q = kLds44BiasQuads + kLds44Ahead;
  for (int l = 0; l + 1 < net.n_layers; l++) q += lds44_quads_of(net.layers[l]);
  return q * 64 * 4;
}

constexpr size_t kLds44MaxBytes = 160 * 1024;  // the dynamic-LDS limit the launchers request

hipError_t launch_rollout_lds44(const NetDesc &net, const RolloutArgs &a, hipStream_t stream)
{
  if (!lds44_supported(net) || a.K % kRolloutsPerWave != 0) return hipErrorInvalidValue;
  const dim3 grid(a.K / kRolloutsPerWave), block(512);
  const int img_f4 = lds44_pack_floats(net) / 4;
  const size_t lds = kM44GroupImageOffset + sizeof(m44_f4) * (size_t)img_f4;
  const M44LayerList nd = m44_layer_list_of(net);
  return dispatch_rollout_flags(a.cost.affine != 0, a.cost.need_control_cost != 0, a.gate != nullptr, [&](auto af, auto ct, auto ga) {
    constexpr auto kern = &rollout_lds44_kernel<decltype(af)::value, decltype(ct)::value, decltype(ga)::value>;
    if (hipError_t e = raise_lds_limit_once<kern>(kLds44MaxBytes); e != hipSuccess) return e;
    MPPI_LAUNCH_ROLLOUT(kern, grid, block, lds, stream, a, nd, img_f4);
    return hipGetLastError();
  });
}

// two instances of ONE layer list (net) in one launch
hipError_t launch_rollout_lds44_batch(const NetDesc &net, const QuadBatchArgs &b, hipStream_t stream)
{
  BatchFlags f;
  if (b.n != 2 || !lds44_supported(net) || !batch_flags_of(b, f)) return hipErrorInvalidValue;
  const QuadBatchArgsT<2> b2 = batch_args_prefix<2>(b);
  const dim3 grid(f.gmax, 2), block(512);
  const int img_f4 = lds44_pack_floats(net) / 4;
  const size_t lds = kM44GroupImageOffset + sizeof(m44_f4) * (size_t)img_f4;
  const M44LayerList nd = m44_layer_list_of(net);
  return dispatch_rollout_flags(f.affine, f.ctrl, f.gated, [&](auto af, auto ct, auto ga) {
    constexpr auto kern = &rollout_lds44_batch_kernel<decltype(af)::value, decltype(ct)::value, decltype(ga)::value, 2>;
    if (hipError_t e = raise_lds_limit_once<kern>(kLds44MaxBytes); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, lds, stream, b2, nd, img_f4);
    return hipGetLastError();
  });
}

}  // namespace mppi
