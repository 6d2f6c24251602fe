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
#include "group_roles.hpp"
#include "m44_core.hpp"
#include "mppi_kernels.hpp"

namespace mppi {

struct Lds44Net {
  int n_layers;
  int layers[8];
};

struct Lds44Shared {
  static constexpr int NW = 4;            // dynamics waves per group, four rollouts each
  static constexpr int NSW = 1;
  static constexpr int kR = 16;
  static constexpr bool kRecByAll = true;
  int xseq[NW][64];
  float rec[kGRing][kRolloutsPerWave][4];
  int cost_done[64];
  float ctl_b1[kGRing][64];
  float ctl_rec[kGRing][kRolloutsPerWave][4];
  int ctl_pub[64];
  float tex[kGRing][kRolloutsPerWave][2];
  int pose_pub[64];
  float eps[kGRing][kRolloutsPerWave][2];
  int rng_pub[64];
  int fail[4];
  int fin[8];
  float gstate[8];   // gated launch: the vehicle state the pose wave took from the gate block, then 1 in gate_open[]
  int gate_open[8];
  float dump[NW][64 * kGRing];  // where the lanes that hold no record word put their copy (never read), per ring slot
};
constexpr size_t kLds44ImageOffset = (sizeof(Lds44Shared) + 15) & ~(size_t)15;

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
__device__ __forceinline__ void lds44_dynamics(const RolloutArgs &a, const Lds44Net &net, Lds44Shared &sh, const m44_f4 *img, const int w)
{
  const int lane = threadIdx.x & 63;
  const int i = lane & 3, row = lane >> 4;
  const int jr = 4 * w + i;  // rollout of the group (A layout: lane-in-quad = rollout)
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

  const uint32_t a_myseq = lds_addr(&sh.xseq[w][lane]);
  typedef const volatile int __attribute__((address_space(3))) *lds_int_p;
  typedef const volatile f32x2 __attribute__((address_space(3))) *lds_f2_p;
  const lds_int_p p_pub = (lds_int_p)&sh.ctl_pub[0];
  const lds_f2_p p_u = (lds_f2_p)&sh.ctl_rec[0][jr][0];  // clamped (u0, u1) of rollout lane & 3, ring slot 0
  constexpr int kSlotF2 = kRolloutsPerWave * 2;
  // the state record: quad 0 of row c holds s[3 + c] of rollouts 0..3; every lane stores (the others into a dump row)
  const uint32_t a_rec0 = ((lane & 12) == 0) ? lds_addr(&sh.rec[0][jr][row]) : lds_addr(&sh.dump[w][lane]);
  constexpr uint32_t kRecStride = sizeof(float) * kRolloutsPerWave * 4;
  static_assert(kRecStride == sizeof(float) * 64, "dump rows move along with the record's ring slot");

  int budget = spin_budget_init(a.spin_budget, T, a.fault_wave == w + 1);
  float sv;
  if constexpr (GATED) {  // the state arrives through the gate block: the pose wave has put it into LDS (group_gate_wait)
    const uint32_t a_go = lds_addr(&sh.gate_open[0]);
    while (lds_peek(a_go) == 0 && --budget > 0) __builtin_amdgcn_s_sleep(1);
    const volatile float *gs = sh.gstate;
    sv = gs[3 + row];
  } else {
    sv = a.state[3 + row];
  }
  while (__builtin_amdgcn_readfirstlane(*p_pub) < 1 && --budget > 0) __builtin_amdgcn_s_sleep(1);
  f32x2 un = p_u[0];
  asm volatile("" : "+v"(un));

  for (int t = 0; t < T - 1; t++) {
    const int slot = t & (kGRing - 1);
    const f32x2 u = un;
    asm volatile("ds_write_b32 %0, %1" ::"v"(a_rec0 + (uint32_t)slot * kRecStride), "v"(sv) : "memory");
    lds_publish(a_myseq, t + 1);  // the record is out; also: this wave is done with the control record of step t
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
    // requested now, used at the end of the step (rollout_row.hip)
    const int sn = ((t + 1) & (kGRing - 1)) * kSlotF2;
    const int cp_v = *p_pub;
    un = p_u[sn];
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
    const int want = t + 2;
    const int cp_e = __builtin_amdgcn_readfirstlane(cp_v);
    asm volatile("" : "+v"(un));
    {
      const float dd = Tr[0] + bo;
      sv = fmaf(dd, a.dt, sv);  // incrementState, neural_net_model.cu:334-344
      asm volatile("" : "+v"(sv));
    }
    if (__builtin_expect(cp_e < want, 0)) {
      int cp = cp_e;
      while (cp < want && --budget > 0) {
        cp = __builtin_amdgcn_readfirstlane(*p_pub);
        un = p_u[sn];
      }
      asm volatile("" : "+v"(un));
    }
  }
  {  // the record of step T-1
    const int t = T - 1;
    asm volatile("ds_write_b32 %0, %1" ::"v"(a_rec0 + (uint32_t)(t & (kGRing - 1)) * kRecStride), "v"(sv) : "memory");
    lds_publish(a_myseq, t + 1);
  }
  spin_finish(budget, lds_addr(&sh.fail[0]), lds_addr(&sh.fin[w]));
}

// one group (workgroup): the four dynamics waves and the four riders; smem: the group's dynamic LDS (Lds44Shared, then the image)
// GATED: enqueued one solve ahead (a.gate != nullptr), state and nominal sequence from the gate block: group_gate_wait
template <bool AFFINE, bool CTRL, bool GATED>
__device__ __forceinline__ void lds44_group(const RolloutArgs &a, const Lds44Net &net, const int img_f4, unsigned char *smem)
{
  using SH = Lds44Shared;
  using RO = GroupRoles<SH>;
  SH &sh = *reinterpret_cast<SH *>(smem);
  m44_f4 *img = reinterpret_cast<m44_f4 *>(smem + kLds44ImageOffset);
  const int lane = threadIdx.x & 63;
  const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  MrgHalf g0{0, 0, 0};
  if (role == RO::kRng) g0 = group_rng_load<SH>(a);
  {  // the image into LDS: it is in LDS order, 16 B per thread and pass
    const m44_f4 *src = reinterpret_cast<const m44_f4 *>(a.wpack);
    for (int q = threadIdx.x; q < img_f4; q += 512) img[q] = src[q];
  }
  if (role == 0) {
#pragma unroll
    for (int w = 0; w < 4; w++) sh.xseq[w][lane] = 0;
    sh.cost_done[lane] = 0;
    sh.ctl_pub[lane] = 0;
    sh.pose_pub[lane] = 0;
    sh.rng_pub[lane] = 0;
    sh.fail[lane & 3] = 0;
    sh.fin[lane & 7] = 0;
    sh.gate_open[lane & 7] = 0;
  }
  __syncthreads();  // the only barrier
  if (role < 4) lds44_dynamics<GATED>(a, net, sh, img, role);
  else if (role == RO::kCost) group_cost_wave4<SH, CTRL>(a, sh);
  else if (role == RO::kCtl) group_control_wave(a, sh, GATED ? lds_addr(&sh.gate_open[0]) : 0u);
  else if (role == RO::kPose) {
    if constexpr (GATED) {
      const int shut = group_gate_wait(a, sh);
      const volatile float *gs = sh.gstate;
      const float x0 = gs[0], y0 = gs[1], yaw0 = gs[2];
      group_pose_wave4<SH, AFFINE>(a, sh, x0, y0, yaw0, shut);
    } else {
      group_pose_wave4<SH, AFFINE>(a, sh);
    }
  }
  else group_rng_wave<SH, true>(a, sh, g0);
}

extern __shared__ __attribute__((aligned(16))) unsigned char lds44_smem[];

template <bool AFFINE, bool CTRL, bool GATED>
__global__ __launch_bounds__(512) void rollout_lds44_kernel(const RolloutArgs a, const Lds44Net net, const int img_f4)
{
  lds44_group<AFFINE, CTRL, GATED>(a, net, img_f4, lds44_smem);
}

// The two controllers of a tick in one launch (mppi_compute_control_batch, mppi_arm_batch): grid (groups of the larger
// instance, 2) -- workgroup (x, y) runs group x of instance y, whose argument block sits at a compile-time position of the
// kernel-argument segment (MPPI_BATCH_DISPATCH, mppi_device.hpp).  All instances have the SAME layer list: one Lds44Net, one
// image size and one dynamic-LDS size serve the launch; each instance copies its own image from its own a.wpack.  GATED: every
// instance's block carries its own handle's gate block (replica blockIdx.x % kGateReplicas: the group index inside the instance).
template <bool AFFINE, bool CTRL, bool GATED, int NB>
__global__ __launch_bounds__(512) void rollout_lds44_batch_kernel(const QuadBatchArgsT<NB> b, const Lds44Net net, const int img_f4)
{
#define MPPI_L44_BODY(A)                                                                                   \
  do {                                                                                                     \
    if ((int)blockIdx.x >= (A).K / kRolloutsPerWave) return; /* the smaller instance of the two */         \
    lds44_group<AFFINE, CTRL, GATED>((A), net, img_f4, lds44_smem);                                        \
  } while (0)
  MPPI_BATCH_DISPATCH(NB, b, MPPI_L44_BODY);
#undef MPPI_L44_BODY
}

// every list 6 -> hidden widths 1..64 -> 4 with at least one hidden layer
bool lds44_supported(const NetDesc &net)
{
  if (net.n_layers < 3 || net.n_layers > 8 || net.layers[0] != kNetIn || net.layers[net.n_layers - 1] != kNetOut) return false;
  for (int l = 1; l + 1 < net.n_layers; l++)
    if (net.layers[l] < 1 || net.layers[l] > 64) return false;
  return true;
}

int lds44_pack_floats(const NetDesc &net)
{
  int q = kLds44BiasQuads + kLds44Ahead;
  for (int l = 0; l + 1 < net.n_layers; l++) q += lds44_quads_of(net.layers[l]);
  return q * 64 * 4;
}

// more dynamic LDS than the default limit: set once per kernel instance and device
#define MPPI_L44_ATTR(KERN)                                                                                            \
  do {                                                                                                                 \
    static bool attr_set[64] = {};                                                                                     \
    if (!attr_set[dev]) {                                                                                              \
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&KERN), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                         160 * 1024);                                                                  \
      if (e != hipSuccess) return e;                                                                                   \
      attr_set[dev] = true;                                                                                            \
    }                                                                                                                  \
  } while (0)

hipError_t launch_rollout_lds44(const NetDesc &net, const RolloutArgs &a, hipStream_t stream)
{
  if (!lds44_supported(net) || a.K % kRolloutsPerWave != 0) return hipErrorInvalidValue;
  const bool affine = a.cost.affine != 0, ctrl = a.cost.need_control_cost != 0, gated = a.gate != nullptr;
  const dim3 grid(a.K / kRolloutsPerWave), block(512);
  const int img_f4 = lds44_pack_floats(net) / 4;
  const size_t lds = kLds44ImageOffset + sizeof(m44_f4) * (size_t)img_f4;
  Lds44Net nd;
  nd.n_layers = net.n_layers;
  for (int i = 0; i < 8; i++) nd.layers[i] = net.layers[i];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
#define MPPI_L44(AF, CT, GA)                                                                                          \
  do {                                                                                                                \
    MPPI_L44_ATTR((rollout_lds44_kernel<AF, CT, GA>));                                                                \
    MPPI_LAUNCH_ROLLOUT((rollout_lds44_kernel<AF, CT, GA>), grid, block, lds, stream, a, nd, img_f4);                 \
  } while (0)
  if (gated) {
    if (affine && !ctrl) MPPI_L44(true, false, true);
    else if (affine && ctrl) MPPI_L44(true, true, true);
    else if (!affine && !ctrl) MPPI_L44(false, false, true);
    else MPPI_L44(false, true, true);
  } else {
    if (affine && !ctrl) MPPI_L44(true, false, false);
    else if (affine && ctrl) MPPI_L44(true, true, false);
    else if (!affine && !ctrl) MPPI_L44(false, false, false);
    else MPPI_L44(false, true, false);
  }
#undef MPPI_L44
  return hipGetLastError();
}

// two instances of ONE layer list (net) in one launch
hipError_t launch_rollout_lds44_batch(const NetDesc &net, const QuadBatchArgs &b, hipStream_t stream)
{
  if (b.n != 2 || !lds44_supported(net)) return hipErrorInvalidValue;
  bool affine = true, ctrl = false;  // the general forms are exact supersets (rollout_mfma.hip)
  int gmax = 0;
  const bool gated = b.inst[0].gate != nullptr;  // mppi_arm_batch: every instance gated on its own block, or none
  for (int i = 0; i < b.n; i++) {
    if ((b.inst[i].gate != nullptr) != gated || b.inst[i].K % kRolloutsPerWave != 0) return hipErrorInvalidValue;
    affine = affine && b.inst[i].cost.affine != 0;
    ctrl = ctrl || b.inst[i].cost.need_control_cost != 0;
    gmax = b.inst[i].K / kRolloutsPerWave > gmax ? b.inst[i].K / kRolloutsPerWave : gmax;
  }
  const QuadBatchArgsT<2> b2 = batch_args_prefix<2>(b);
  const dim3 grid(gmax, 2), block(512);
  const int img_f4 = lds44_pack_floats(net) / 4;
  const size_t lds = kLds44ImageOffset + sizeof(m44_f4) * (size_t)img_f4;
  Lds44Net nd;
  nd.n_layers = net.n_layers;
  for (int i = 0; i < 8; i++) nd.layers[i] = net.layers[i];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
#define MPPI_L44B(AF, CT, GA)                                                                                         \
  do {                                                                                                                \
    MPPI_L44_ATTR((rollout_lds44_batch_kernel<AF, CT, GA, 2>));                                                       \
    hipLaunchKernelGGL((rollout_lds44_batch_kernel<AF, CT, GA, 2>), grid, block, lds, stream, b2, nd, img_f4);        \
  } while (0)
  if (gated) {
    if (affine && !ctrl) MPPI_L44B(true, false, true);
    else if (affine && ctrl) MPPI_L44B(true, true, true);
    else if (!affine && !ctrl) MPPI_L44B(false, false, true);
    else MPPI_L44B(false, true, true);
  } else {
    if (affine && !ctrl) MPPI_L44B(true, false, false);
    else if (affine && ctrl) MPPI_L44B(true, true, false);
    else if (!affine && !ctrl) MPPI_L44B(false, false, false);
    else MPPI_L44B(false, true, false);
  }
#undef MPPI_L44B
  return hipGetLastError();
}
#undef MPPI_L44_ATTR

}  // namespace mppi
