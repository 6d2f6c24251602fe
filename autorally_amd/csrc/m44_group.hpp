// m44_group.hpp -- the GROUP of the forms on v_mfma_f32_4x4x1 with A-matrix broadcast (rollout_m44.hip, rollout_lds44.hip,
// rollout_lds128.hip): 512 threads per 16 rollouts, 4 dynamics waves x 4 rollouts + the four riders of group_roles.hpp,
// record rings in LDS, one barrier.  Here, once: the group's shared state, the layer list the lds forms take as a kernel
// argument, the dynamics wave's side of the hand-overs with the riders (M44Wave) and the group body (m44_group_body).  A
// form adds its network: where its weights are staged in front of the barrier and what a dynamics wave computes between
// M44Wave's pieces.
#pragma once
#include "group_roles.hpp"
#include "m44_core.hpp"
#include "mppi_kernels.hpp"

namespace mppi {

struct M44GroupShared {
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

// The lds forms: the group's dynamic LDS is the shared state, then the weight image; the layer list is a kernel argument.
constexpr size_t kM44GroupImageOffset = (sizeof(M44GroupShared) + 15) & ~(size_t)15;
extern __shared__ __attribute__((aligned(16))) unsigned char m44_group_smem[];
struct M44LayerList {
  int n_layers;
  int layers[8];
};
inline M44LayerList m44_layer_list_of(const NetDesc &net)
{
  M44LayerList nd;
  nd.n_layers = net.n_layers;
  for (int i = 0; i < 8; i++) nd.layers[i] = net.layers[i];
  return nd;
}

// A dynamics wave's side of the hand-overs: the state record and the sequence word it publishes per step, the clamped
// controls it takes from the control wave, the poll budget all its waits share.  A form's dynamics function reads
//   M44Wave<GATED> wv(a, sh, w);
//   for (t = 0 .. T - 2) { u = wv.open(t); sv = wv.sv; <layer 0>; wv.request(t + 1); <the other layers>; wv.close(t, a.dt, <output>); }
//   wv.finish(T - 1, sh, w);
// with the state entry s[3 + row] of rollout lane & 3 in wv.sv (row c of the wave = lanes 16 c ..).
// The pieces are optimised once on their own before they are inlined, with the members still in memory: a piece counts its
// polls in a local and stores the budget once, and a form reads wv.sv once per step into a local of its own.  With that the
// kernels' instruction streams are those of the skeleton written out in each form (profiles/r15_a_m44_family_isa.txt).
template <bool GATED>
struct M44Wave {
  typedef const volatile int __attribute__((address_space(3))) *lds_int_p;
  typedef const volatile f32x2 __attribute__((address_space(3))) *lds_f2_p;
  static constexpr int kSlotF2 = kRolloutsPerWave * 2;
  static constexpr uint32_t kRecStride = sizeof(float) * kRolloutsPerWave * 4;
  static_assert(kRecStride == sizeof(float) * 64, "dump rows move along with the record's ring slot");
  uint32_t a_myseq, a_rec0;
  lds_int_p p_pub;
  lds_f2_p p_u;  // clamped (u0, u1) of rollout lane & 3, ring slot 0
  int budget, sn, cp_v;
  float sv;
  f32x2 un;

  // set-up: the addresses, the state (GATED: once the pose wave has put it into LDS, group_gate_wait), the first controls
  __device__ __forceinline__ M44Wave(const RolloutArgs &a, M44GroupShared &sh, const int w)
  {
    const int lane = threadIdx.x & 63;
    const int row = lane >> 4;
    const int jr = 4 * w + (lane & 3);  // rollout of the group (A layout: lane-in-quad = rollout)
    a_myseq = lds_addr(&sh.xseq[w][lane]);
    p_pub = (lds_int_p)&sh.ctl_pub[0];
    p_u = (lds_f2_p)&sh.ctl_rec[0][jr][0];
    // the state record: quad 0 of row c holds s[3 + c] of rollouts 0..3; every lane stores (the others into a dump row)
    a_rec0 = ((lane & 12) == 0) ? lds_addr(&sh.rec[0][jr][row]) : lds_addr(&sh.dump[w][lane]);
    int left = spin_budget_init(a.spin_budget, a.T, a.fault_wave == w + 1);
    if constexpr (GATED) {
      const uint32_t a_go = lds_addr(&sh.gate_open[0]);
      while (lds_peek(a_go) == 0 && --left > 0) __builtin_amdgcn_s_sleep(1);
      const volatile float *gs = sh.gstate;
      sv = gs[3 + row];
    } else {
      sv = a.state[3 + row];
    }
    while (__builtin_amdgcn_readfirstlane(*p_pub) < 1 && --left > 0) __builtin_amdgcn_s_sleep(1);
    budget = left;
    un = p_u[0];
    asm volatile("" : "+v"(un));
  }
  __device__ __forceinline__ void put_record(const int t)
  {
    asm volatile("ds_write_b32 %0, %1" ::"v"(a_rec0 + (uint32_t)(t & (kGRing - 1)) * kRecStride), "v"(sv) : "memory");
    lds_publish(a_myseq, t + 1);  // the record is out; also: this wave is done with the control record of step t
  }
  // the record of step t goes out; returns the controls of step t
  __device__ __forceinline__ f32x2 open(const int t)
  {
    const f32x2 u = un;
    put_record(t);
    return u;
  }
  // the controls of step tn = t + 1: requested now (behind layer 0), used at the end of the step (rollout_row.hip)
  __device__ __forceinline__ void request(const int tn)
  {
    sn = (tn & (kGRing - 1)) * kSlotF2;
    cp_v = *p_pub;
    un = p_u[sn];
  }
  // the state update with the form's output (out() = the derivative of this lane's state entry), then the controls of step
  // t + 1: they are there unless the control wave has fallen behind (the cold loop)
  __device__ __forceinline__ void close(const int t, const float dt, const float dd)
  {
    const int want = t + 2;
    const int cp_e = __builtin_amdgcn_readfirstlane(cp_v);
    asm volatile("" : "+v"(un));
    sv = fmaf(dd, dt, sv);  // incrementState, neural_net_model.cu:334-344
    asm volatile("" : "+v"(sv));
    if (__builtin_expect(cp_e < want, 0)) {
      int cp = cp_e, left = budget;
      while (cp < want && --left > 0) {
        cp = __builtin_amdgcn_readfirstlane(*p_pub);
        un = p_u[sn];
      }
      budget = left;
      asm volatile("" : "+v"(un));
    }
  }
  // the record of the last step, then the fail and finished words
  __device__ __forceinline__ void finish(const int t, M44GroupShared &sh, const int w)
  {
    put_record(t);
    spin_finish(budget, lds_addr(&sh.fail[0]), lds_addr(&sh.fin[w]));
  }
};

// One group (workgroup): the four dynamics waves and the four riders.  FORM provides
//   typename Shared                       M44GroupShared, or a struct derived from it
//   stage_by_all(a, sh)                   what all 512 threads put into LDS in front of the barrier (the lds forms: the image)
//   stage_by_wave1(a, sh)                 what wave 1 puts there (m44: the output layer's weights)
//   dynamics<GATED>(a, sh, w)             dynamics wave w
// GATED: enqueued one solve ahead (a.gate != nullptr), state and nominal sequence from the gate block: group_gate_wait
template <bool AFFINE, bool CTRL, bool GATED, class FORM>
__device__ __forceinline__ void m44_group_body(const RolloutArgs &a, typename FORM::Shared &sh, const FORM &form)
{
  using SH = typename FORM::Shared;
  using RO = GroupRoles<SH>;
  const int lane = threadIdx.x & 63;
  const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  MrgHalf g0{0, 0, 0};
  if (role == RO::kRng) g0 = group_rng_load<SH>(a);
  form.stage_by_all(a, sh);
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
  if (role == 1) form.stage_by_wave1(a, sh);
  __syncthreads();  // the only barrier
  if (role < 4) form.template dynamics<GATED>(a, sh, role);
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

// The two controllers of a tick in one launch (mppi_compute_control_batch, mppi_arm_batch): grid (groups of the larger
// instance, 2) -- workgroup (x, y) runs group x of instance y, whose argument block sits at a compile-time position of the
// kernel-argument segment (MPPI_BATCH_DISPATCH, mppi_device.hpp: the body reads its parameters as the single-instance
// kernel does, not through scratch).  Every block carries its own wpack and generator state: an instance's bits are those
// of its own launch.  GATED: every instance's block carries its OWN handle's gate block, whose pose wave polls replica
// blockIdx.x % kGateReplicas of it -- blockIdx.x is the group index inside the instance, as in the single gated kernel.
template <bool AFFINE, bool CTRL, bool GATED, int NB, class FORM>
__device__ __forceinline__ void m44_group_batch_body(const QuadBatchArgsT<NB> &b, typename FORM::Shared &sh, const FORM &form)
{
#define MPPI_M44_BODY(A)                                                                                   \
  do {                                                                                                     \
    if ((int)blockIdx.x >= (A).K / kRolloutsPerWave) return; /* the smaller instance of the two */         \
    m44_group_body<AFFINE, CTRL, GATED>((A), sh, form);                                                    \
  } while (0)
  MPPI_BATCH_DISPATCH(NB, b, MPPI_M44_BODY);
#undef MPPI_M44_BODY
}

// An lds form: the image (a.wpack, img_f4 float4 in LDS order) behind the shared state, copied by all threads, 16 B per thread
// and pass; DYN(a, net, sh, img, w) is the form's dynamics wave (its GATED instance: the kernel names it)
template <auto DYN>
struct M44LdsForm {
  using Shared = M44GroupShared;
  const M44LayerList &net;
  const int img_f4;
  __device__ __forceinline__ m44_f4 *image() const { return reinterpret_cast<m44_f4 *>(m44_group_smem + kM44GroupImageOffset); }
  __device__ __forceinline__ void stage_by_all(const RolloutArgs &a, Shared &) const
  {
    m44_f4 *img = image();
    const m44_f4 *src = reinterpret_cast<const m44_f4 *>(a.wpack);
    for (int q = threadIdx.x; q < img_f4; q += 512) img[q] = src[q];
  }
  __device__ __forceinline__ void stage_by_wave1(const RolloutArgs &, Shared &) const {}
  template <bool GATED>
  __device__ __forceinline__ void dynamics(const RolloutArgs &a, Shared &sh, const int w) const
  {
    DYN(a, net, sh, image(), w);
  }
};
template <auto DYN, bool AFFINE, bool CTRL, bool GATED>
__device__ __forceinline__ void m44_lds_kernel_body(const RolloutArgs &a, const M44LayerList &net, const int img_f4)
{
  m44_group_body<AFFINE, CTRL, GATED>(a, *reinterpret_cast<M44GroupShared *>(m44_group_smem), M44LdsForm<DYN>{net, img_f4});
}
// All instances have the SAME layer list: one M44LayerList, one image size and one dynamic-LDS size serve the launch; each
// instance copies its own image from its own a.wpack.
template <auto DYN, bool AFFINE, bool CTRL, bool GATED, int NB>
__device__ __forceinline__ void m44_lds_batch_kernel_body(const QuadBatchArgsT<NB> &b, const M44LayerList &net, const int img_f4)
{
  m44_group_batch_body<AFFINE, CTRL, GATED, NB>(b, *reinterpret_cast<M44GroupShared *>(m44_group_smem), M44LdsForm<DYN>{net, img_f4});
}

}  // namespace mppi
