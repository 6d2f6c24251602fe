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
#include "group_roles.hpp"
#include "m44_core.hpp"
#include "mppi_kernels.hpp"

namespace mppi {

struct Lds128Net {
  int n_layers;
  int layers[8];
};

// rollout_lds44.hip's shared state, member by member (GroupRoles reads it by name)
struct Lds128Shared {
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
constexpr size_t kLds128ImageOffset = (sizeof(Lds128Shared) + 15) & ~(size_t)15;
constexpr size_t kLds128MaxBytes = 160 * 1024;  // the dynamic-LDS limit the launcher requests

__host__ __device__ inline int lds128_quads_of(int nin) { return (nin + 3) >> 2; }
__host__ __device__ inline int lds128_halves_of(int nout) { return nout > 64 ? 2 : 1; }

// The read-ahead is requested HERE: without this the compiler moves a request behind the wave-uniform exit in front of its
// use and waits for every quad (no instruction, no wait: a compiler barrier for memory operations only)
__device__ __forceinline__ void lds128_pin_reads() { asm volatile("" ::: "memory"); }

// one half per layer (and the output layer): stream element Q is quad Q of the ONE accumulator; quads 16.. read T1
template <int Q>
__device__ __forceinline__ void lds128_chain1(m44_f4 &d, const float (&T0)[4], const float (&T1)[4], m44_f4 (&w)[kLds44Ahead],
                                              const m44_f4 *p, const int nq)
{
  if constexpr (Q < 32) {
    if (Q > 0 && Q >= nq) return;  // wave-uniform
    const m44_f4 x = w[Q % kLds44Ahead];
    if constexpr (Q + kLds44Ahead < 32) w[Q % kLds44Ahead] = p[(Q + kLds44Ahead) * 64];
    lds128_pin_reads();
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
    lds128_pin_reads();
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
__device__ __forceinline__ void lds128_dynamics(const RolloutArgs &a, const Lds128Net &net, Lds128Shared &sh, const m44_f4 *img, const int w)
{
  const int lane = threadIdx.x & 63;
  const int i = lane & 3, row = lane >> 4;
  const int jr = 4 * w + i;  // rollout of the group (A layout: lane-in-quad = rollout)
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
    // requested now, used at the end of the step (rollout_row.hip)
    const int sn = ((t + 1) & (kGRing - 1)) * kSlotF2;
    const int cp_v = *p_pub;
    un = p_u[sn];
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
    const int want = t + 2;
    const int cp_e = __builtin_amdgcn_readfirstlane(cp_v);
    asm volatile("" : "+v"(un));
    {
      const float dd = T0[0] + bo;
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

// one group (workgroup): the four dynamics waves and the four riders; smem: the group's dynamic LDS (Lds128Shared, then the image)
// GATED: enqueued one solve ahead (a.gate != nullptr), state and nominal sequence from the gate block: group_gate_wait
template <bool AFFINE, bool CTRL, bool GATED>
__device__ __forceinline__ void lds128_group(const RolloutArgs &a, const Lds128Net &net, const int img_f4, unsigned char *smem)
{
  using SH = Lds128Shared;
  using RO = GroupRoles<SH>;
  SH &sh = *reinterpret_cast<SH *>(smem);
  m44_f4 *img = reinterpret_cast<m44_f4 *>(smem + kLds128ImageOffset);
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
  if (role < 4) lds128_dynamics<GATED>(a, net, sh, img, role);
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

extern __shared__ __attribute__((aligned(16))) unsigned char lds128_smem[];

template <bool AFFINE, bool CTRL, bool GATED>
__global__ __launch_bounds__(512) void rollout_lds128_kernel(const RolloutArgs a, const Lds128Net net, const int img_f4)
{
  lds128_group<AFFINE, CTRL, GATED>(a, net, img_f4, lds128_smem);
}

// The two controllers of a tick in one launch (mppi_compute_control_batch, mppi_arm_batch), as rollout_lds44_batch_kernel:
// grid (groups of the larger instance, 2), workgroup (x, y) runs group x of instance y.  All instances have the SAME layer
// list: one Lds128Net, one image size and one dynamic-LDS size serve the launch; each instance copies its own image.
template <bool AFFINE, bool CTRL, bool GATED, int NB>
__global__ __launch_bounds__(512) void rollout_lds128_batch_kernel(const QuadBatchArgsT<NB> b, const Lds128Net net, const int img_f4)
{
#define MPPI_L128_BODY(A)                                                                                  \
  do {                                                                                                     \
    if ((int)blockIdx.x >= (A).K / kRolloutsPerWave) return; /* the smaller instance of the two */         \
    lds128_group<AFFINE, CTRL, GATED>((A), net, img_f4, lds128_smem);                                      \
  } while (0)
  MPPI_BATCH_DISPATCH(NB, b, MPPI_L128_BODY);
#undef MPPI_L128_BODY
}

int lds128_pack_floats(const NetDesc &net)
{
  int q = kLds128BiasQuads + kLds44Ahead;
  const int n_w = net.n_layers - 1;
  for (int j = 0; j < n_w; j++) q += lds128_quads_of(net.layers[j]) * (j + 1 < n_w ? lds128_halves_of(net.layers[j + 1]) : 1);
  return q * 64 * 4;
}

static bool lds128_list_ok(const NetDesc &net)
{
  if (net.n_layers < 3 || net.n_layers > 8 || net.layers[0] != kNetIn || net.layers[net.n_layers - 1] != kNetOut) return false;
  for (int l = 1; l + 1 < net.n_layers; l++)
    if (net.layers[l] < 1 || net.layers[l] > 128) return false;
  return true;
}

// the group's dynamic LDS: shared state + image; 0 for a list the form does not take whatever its size
size_t lds128_lds_bytes(const NetDesc &net)
{
  if (!lds128_list_ok(net)) return 0;
  return kLds128ImageOffset + sizeof(float) * (size_t)lds128_pack_floats(net);
}
size_t lds128_lds_limit() { return kLds128MaxBytes; }

// every list 6 -> hidden widths 1..128 -> 4 with at least one hidden layer whose image fits one workgroup's LDS
bool lds128_supported(const NetDesc &net) { return lds128_list_ok(net) && lds128_lds_bytes(net) <= kLds128MaxBytes; }

// more dynamic LDS than the default limit: set once per kernel instance and device
#define MPPI_L128_ATTR(KERN)                                                                                           \
  do {                                                                                                                 \
    static bool attr_set[64] = {};                                                                                     \
    if (!attr_set[dev]) {                                                                                              \
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&KERN), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                         (int)kLds128MaxBytes);                                                        \
      if (e != hipSuccess) return e;                                                                                   \
      attr_set[dev] = true;                                                                                            \
    }                                                                                                                  \
  } while (0)

hipError_t launch_rollout_lds128(const NetDesc &net, const RolloutArgs &a, hipStream_t stream)
{
  if (!lds128_supported(net) || a.K % kRolloutsPerWave != 0) return hipErrorInvalidValue;
  const bool affine = a.cost.affine != 0, ctrl = a.cost.need_control_cost != 0, gated = a.gate != nullptr;
  const dim3 grid(a.K / kRolloutsPerWave), block(512);
  const int img_f4 = lds128_pack_floats(net) / 4;
  const size_t lds = lds128_lds_bytes(net);
  Lds128Net nd;
  nd.n_layers = net.n_layers;
  for (int i = 0; i < 8; i++) nd.layers[i] = net.layers[i];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
#define MPPI_L128(AF, CT, GA)                                                                                         \
  do {                                                                                                                \
    MPPI_L128_ATTR((rollout_lds128_kernel<AF, CT, GA>));                                                              \
    MPPI_LAUNCH_ROLLOUT((rollout_lds128_kernel<AF, CT, GA>), grid, block, lds, stream, a, nd, img_f4);                \
  } while (0)
  if (gated) {
    if (affine && !ctrl) MPPI_L128(true, false, true);
    else if (affine && ctrl) MPPI_L128(true, true, true);
    else if (!affine && !ctrl) MPPI_L128(false, false, true);
    else MPPI_L128(false, true, true);
  } else {
    if (affine && !ctrl) MPPI_L128(true, false, false);
    else if (affine && ctrl) MPPI_L128(true, true, false);
    else if (!affine && !ctrl) MPPI_L128(false, false, false);
    else MPPI_L128(false, true, false);
  }
#undef MPPI_L128
  return hipGetLastError();
}

// two instances of ONE layer list (net) in one launch
hipError_t launch_rollout_lds128_batch(const NetDesc &net, const QuadBatchArgs &b, hipStream_t stream)
{
  if (b.n != 2 || !lds128_supported(net)) return hipErrorInvalidValue;
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
  const int img_f4 = lds128_pack_floats(net) / 4;
  const size_t lds = lds128_lds_bytes(net);
  Lds128Net nd;
  nd.n_layers = net.n_layers;
  for (int i = 0; i < 8; i++) nd.layers[i] = net.layers[i];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
#define MPPI_L128B(AF, CT, GA)                                                                                        \
  do {                                                                                                                \
    MPPI_L128_ATTR((rollout_lds128_batch_kernel<AF, CT, GA, 2>));                                                     \
    hipLaunchKernelGGL((rollout_lds128_batch_kernel<AF, CT, GA, 2>), grid, block, lds, stream, b2, nd, img_f4);       \
  } while (0)
  if (gated) {
    if (affine && !ctrl) MPPI_L128B(true, false, true);
    else if (affine && ctrl) MPPI_L128B(true, true, true);
    else if (!affine && !ctrl) MPPI_L128B(false, false, true);
    else MPPI_L128B(false, true, true);
  } else {
    if (affine && !ctrl) MPPI_L128B(true, false, false);
    else if (affine && ctrl) MPPI_L128B(true, true, false);
    else if (!affine && !ctrl) MPPI_L128B(false, false, false);
    else MPPI_L128B(false, true, false);
  }
#undef MPPI_L128B
  return hipGetLastError();
}
#undef MPPI_L128_ATTR

}  // namespace mppi
