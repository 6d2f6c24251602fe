// row_group.hpp -- the ROW group: the latency form of layer lists up to 32 wide on the VECTOR ALU, four rollouts per dynamics
// wavefront (a rollout = one 16-lane DPP row, lane p owns neurons 2p, 2p+1 of every hidden layer, every weight in registers),
// four dynamics wavefronts + the four riders of group_roles.hpp per 16 rollouts.  What the form is and why is written down at the
// top of rollout_row.hip, whose kernels (6-32-32-4: NHH = 1) are instances of this text; rollout_row32.hip instantiates the
// other depths.
//
// NHH = hidden layers - 1 in {0, 1, 2, 3}: the number of 32 x 32 hidden-to-hidden layers, each one more row_dot_bc chain and one
// more tanh_bias2 per step and 32 more register pairs per lane.  With NHH = 0 the output layer reads layer 0's activations.
// VGPRs (tree / exact): NHH 0: 40-48 / 98-104, 1: 107 / 165, 2: 173-174 / 231-236, 3: 239-240 / does not fit (spills: not built).
// From NHH = 2 on a 512-thread group is alone on its CU.
//
// A hidden layer NARROWER than 32 runs as a 32-wide one (pack_row32_weights, abi_pack.hip): the neurons it does not have carry
// weight 0 and bias 0, and the next layer's weights for them are 0.  tanh_bias2(0, 0) is exactly 0, and the padded inputs come
// LAST in every chain, so the real part of a chain is the reference's k-ascending chain and the padded tail adds (+0) x (+0) to
// it.  The one thing that can change is the SIGN OF A ZERO: a pre-activation whose real chain ends at exactly -0 leaves the padded
// tail as +0 (-0 + +0 = +0).  With a bias that is not zero -- every trained model -- no sum stays at -0.
#pragma once
#include "group_roles.hpp"
#include "mppi_kernels.hpp"

// rollout_row.hip's diagnostic build (-DMPPI_ROW_STAMPS) defines the stamps in front of this header; the product has none
#ifndef RSTAMP
#define RSTAMP(i) do { } while (0)
#endif

namespace mppi {

template <int H>
struct RowShared {
  static constexpr int NW = 4;            // dynamics waves per group, four rollouts each
  static constexpr int NSW = 1;           // xseq[w] = steps published by dynamics wave w
  static constexpr bool kRecByAll = true; // every dynamics wave writes the state records of its own rollouts
  static constexpr int kR = 16;           // rollouts per group
  int xseq[NW][64];
  float rec[kGRing][kRolloutsPerWave][4];   // s3..s6 before the update of step t; also the layer-0 input of that step
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
  float gstate[8];  // gated launch: the vehicle state the pose wave took from the gate block, then 1 in gate_open[]
  int gate_open[8];
  float dump[NW][64 * 2 + (kGRing - 1) * kRolloutsPerWave * 4];  // where lanes p >= 2 of a dynamics wave put their copy of the state
                                                                 // pair (never read): 8 B per lane, moved along with the ring slot
};

// TREE (the "row_tree" form): the output layer as own-activation partials + a butterfly over the row instead of the
// k-ascending chain -- see row_out_tree below; w3 then holds this lane's 2 x 4 output weights instead of all 32 x 2.
template <int H, bool TREE, int NHH>
struct RowWeights {
  static constexpr int NA = NHH > 0 ? NHH : 1;  // (no array of zero elements)
  f32x2 w1[kNetIn], w2[NA][H], w3[TREE ? 4 : H];
  f32x2 b1s, b2s[NA], b3;  // hidden biases pre-scaled for tanh_bias2 (theta_s of the register VALU kernel)
};

// rowpack: the weights in REGISTER order, written by the host (pack_row_weights, pack_row32_weights, abi_pack.hip): 16-B entry i
// of lane p at float4 index i * 16 + p -- a load instruction of a wave reads 256 contiguous bytes (the four rollouts of a wave
// share them).  Entries (row_pack_layout, mppi_kernels.hpp), E = 3 + 16 NHH: 0..2 = w1[0..5]; 3 + 16 l .. 18 + 16 l = the
// hidden-to-hidden layer l < NHH, w2[l][0..31]; E .. E + 15 = w3[0..31] (pairs, two per entry); then (NHH + 2) / 2 entries of
// hidden biases, two layers per entry: (b1s, b2s[0]), (b2s[1], b2s[2]); then b3.
// Tree form, behind b3: (W3[o][2p], W3[o^1][2p], W3[o][2p+1], W3[o^1][2p+1]), the same of outputs o^2, o^3, (b3[o], -, -, -),
// o = p >> 2 the output this lane's quad ends up with.
// NHH = 1 is pack_row_weights' image entry for entry: 3..18 = w2, 19..34 = w3, 35 = (b1s, b2s), 36 = b3, 37..39 the tree's.
// (Loading the rows straight from the packed theta -- 44 scattered 16-B loads per lane -- cost 2.1 us per launch.)
template <int H, bool TREE, int NHH>
__device__ __forceinline__ void row_load(const float *rowpack, int p, RowWeights<H, TREE, NHH> &W)
{
  static_assert(H == 32, "entry layout of pack_row_weights");
  constexpr RowPackLayout E = row_pack_layout(NHH);
  const float4 *pk = reinterpret_cast<const float4 *>(rowpack) + p;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float4 v = pk[i * 16];
    W.w1[2 * i] = f32x2{v.x, v.y};
    W.w1[2 * i + 1] = f32x2{v.z, v.w};
  }
#pragma unroll
  for (int i = 0; i < H / 2; i++) {
#pragma unroll
    for (int l = 0; l < NHH; l++) {
      const float4 v = pk[(E.w2 + l * (H / 2) + i) * 16];
      W.w2[l][2 * i] = f32x2{v.x, v.y};
      W.w2[l][2 * i + 1] = f32x2{v.z, v.w};
    }
    if constexpr (!TREE) {
      const float4 u = pk[(E.w3 + i) * 16];
      W.w3[2 * i] = f32x2{u.x, u.y};
      W.w3[2 * i + 1] = f32x2{u.z, u.w};
    }
  }
  const float4 b = pk[E.bias * 16];
  W.b1s = f32x2{b.x, b.y};
  if constexpr (NHH >= 1) W.b2s[0] = f32x2{b.z, b.w};
  if constexpr (NHH >= 2) {
    const float4 b2 = pk[(E.bias + 1) * 16];
    W.b2s[1] = f32x2{b2.x, b2.y};
    if constexpr (NHH >= 3) W.b2s[2] = f32x2{b2.z, b2.w};
  }
  if constexpr (TREE) {
    const float4 u = pk[E.tree * 16], v = pk[(E.tree + 1) * 16], c = pk[(E.tree + 2) * 16];
    W.w3[0] = f32x2{u.x, u.y};
    W.w3[1] = f32x2{u.z, u.w};
    W.w3[2] = f32x2{v.x, v.y};
    W.w3[3] = f32x2{v.z, v.w};
    W.b3 = f32x2{c.x, c.y};
  } else {
    const float4 c = pk[E.b3 * 16];
    W.b3 = f32x2{c.x, c.y};
  }
}

// A value of this lane's rollout from the registers of the lane that holds it: a rollout is one 16-lane DPP row,
// `row_newbcast:q` hands every lane of a row the value of lane q (off the dependent chain).  gfx90a+ DPP control 0x150 + q;
// works on 32-bit operands on gfx950 (tools/ub/row_bcast_ub.hip checks the bits against the LDS form) and on 64-bit ones
// (row_bc2 below).  This 32-bit form brings the state components to layer 0.
template <int Q>
__device__ __forceinline__ float row_bc(float a)
{
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(a), 0x150 + Q, 0xF, 0xF, false));
}
// z = sum_k w[k] * a[k] over the 32 activations of the rollout (lane q holds a[2q], a[2q+1]), k ascending: ONE chain of
// dependent v_pk_fma_f32 (8.5 cycles apart, tools/ub/valu_issue_ub.hip).  The PAIR of lane q comes by one v_mov_b64_dpp
// `row_newbcast:q` (the 64-bit move takes the same DPP control) and serves the multiply-adds of k = 2q (both halves read
// the pair's low word: op_sel) and k = 2q+1 (the high word): 16 moves + 32 multiply-adds per layer instead of 32 + 32 with
// 32-bit moves -- the same arithmetic bit for bit, rollout 36.9 -> 34.3 us, step 0.0486 -> 0.0461 ms
// (profiles/r04_r_mov64_ab.txt).  Written as the schedule it has to be -- multiply-add of 2q, the move for q+1 in its
// shadow, multiply-add of 2q+1 -- and held there by scheduling barriers (left alone inside the kernel, the scheduler hoists
// all moves in front of the chain: ~130 cycles more per layer).
template <int Q>
__device__ __forceinline__ f32x2 row_bc2(f32x2 a)
{
  return __builtin_bit_cast(f32x2, (long long)__builtin_amdgcn_mov_dpp(__builtin_bit_cast(long long, a), 0x150 + Q, 0xF, 0xF, false));
}
template <int Q>
__device__ __forceinline__ void row_dot_step(f32x2 &z, f32x2 &b, const f32x2 *w, f32x2 a)
{
  z = __builtin_elementwise_fma(w[2 * Q], f32x2{b.x, b.x}, z);
  __builtin_amdgcn_sched_barrier(0);
  const f32x2 bn = row_bc2<(Q + 1 < 16 ? Q + 1 : 15)>(a);
  __builtin_amdgcn_sched_barrier(0);
  z = __builtin_elementwise_fma(w[2 * Q + 1], f32x2{b.y, b.y}, z);
  __builtin_amdgcn_sched_barrier(0);
  b = bn;
}
__device__ __forceinline__ f32x2 row_dot_bc(const f32x2 *w, f32x2 a)
{
  f32x2 z = {0.0f, 0.0f};
  f32x2 b = row_bc2<0>(a);
  __builtin_amdgcn_sched_barrier(0);
#define RD4(Q) row_dot_step<Q>(z, b, w, a); row_dot_step<Q + 1>(z, b, w, a); row_dot_step<Q + 2>(z, b, w, a); row_dot_step<Q + 3>(z, b, w, a);
  RD4(0) RD4(4) RD4(8) RD4(12)
#undef RD4
  return z;
}

// The output layer of the TREE form ("row_tree").  In the exact form every lane of a rollout runs the whole 32-long chain
// for two of the four outputs -- 32 dependent packed multiply-adds and 32 moves per lane and step, ~290 of the step's ~930
// cycles and 30 % of the kernel's vector instructions, for 4 useful numbers.  Here lane p multiplies only ITS OWN two
// activations (a[2p], a[2p+1]) into the four outputs (a product and a fused multiply-add each, packed: 4 instructions) and
// the 16 partials of an output are summed by a butterfly of DPP adds that halves the number of live values per level:
//   level 1 (row_ror:8):        v0 += v2(p^8), v1 += v3(p^8)    lanes p < 8 keep outputs {0,1}, lanes p >= 8 outputs {2,3}
//   level 2 (row_half_mirror):  v0 += v1(p^7)                   quad q = p >> 2 keeps output q
//   level 3, 4 (quad_perm):     v0 += v0(p^1); v0 += v0(p^2)
// -- 5 adds on a 4-deep chain; which output a lane keeps is wired into the ORDER of its weights (v_i = partial of output
// (p >> 2) ^ i, pack_row_weights), so no select is needed.  Every lane of quad q ends with output q = state component
// s[3 + q]: layer 0 of the next step takes the state from lanes 0, 4, 8, 12 of the row.  This is NOT the reference's
// summation order (neural_net_model.cu:379-394 sums k ascending; the hidden layers keep that order): the form is opt-in by
// tolerance -- checked bit for bit against the test oracle's mode 2 (its out_tree_dot), and against the
// nominal oracle at the north-star criteria (controls 1e-4).
template <int CTRL>
__device__ __forceinline__ float dpp_add(float acc, float src)
{
  return acc + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(src), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row_out_tree(const f32x2 *w3, f32x2 a)
{
  const f32x2 ax = {a.x, a.x}, ay = {a.y, a.y};
  const f32x2 v01 = __builtin_elementwise_fma(w3[1], ay, w3[0] * ax);
  const f32x2 v23 = __builtin_elementwise_fma(w3[3], ay, w3[2] * ax);
  float v0 = dpp_add<0x128>(v01.x, v23.x);  // row_ror:8
  const float v1 = dpp_add<0x128>(v01.y, v23.y);
  v0 = dpp_add<0x141>(v0, v1);              // row_half_mirror: lane p <- lane p ^ 7
  v0 = dpp_add<0xB1>(v0, v0);               // quad_perm [1,0,3,2]
  v0 = dpp_add<0x4E>(v0, v0);               // quad_perm [2,3,0,1]
  return v0;
}

// One network step of a dynamics wave, at position Q of its aligned chunk of four steps [t0, t0 + 4) -- the T loop of
// row_dynamics below is this body four times.  What a step does besides the network is wired to Q at compile time:
//   * ring slots: slot (t0 + Q) % kGRing = (t0 % kGRing) + Q never wraps inside an aligned chunk, so the state record goes to
//     the chunk's address a_rec plus Q slots and the controls of step t + 1 come from the chunk's pointer pu plus Q + 1
//     slots, both in the `offset:` field of the LDS instruction.  Only the read of Q = 3 leaves the chunk: it moves pu on
//     to the next chunk (the one address add of a chunk besides a_rec's);
//   * the sequence word is published by Q = 3 only, with value t0 + 4 (see the hand-over invariants at row_dynamics);
//   * the control wave's count is READ by Q = 0 only, into the SGPR cp every step of the chunk tests.
template <int H, bool TREE, int NHH, int Q>
__device__ __forceinline__ void row_step(const RolloutArgs &a, const RowWeights<H, TREE, NHH> &W, f32x2 &sp, f32x2 &un, const int t0,
                                         const uint32_t a_rec, const uint32_t a_myseq, const volatile int __attribute__((address_space(3))) *p_pub,
                                         const volatile f32x2 __attribute__((address_space(3))) *&pu,
                                         const volatile f32x2 __attribute__((address_space(3))) *p_u0, int &cp, int &budget)
{
  constexpr int kSlotF2 = kRolloutsPerWave * 2;  // f32x2 per ring slot of ctl_rec (and of rec)
  constexpr uint32_t kRecStride = sizeof(float) * kRolloutsPerWave * 4;
  const int t = t0 + Q;
  const f32x2 u = un;
  const f32x2 slo = TREE ? f32x2{row_bc<0>(sp.x), row_bc<4>(sp.x)} : f32x2{row_bc<0>(sp.x), row_bc<0>(sp.y)};    // (s3, s4)
  const f32x2 shi = TREE ? f32x2{row_bc<8>(sp.x), row_bc<12>(sp.x)} : f32x2{row_bc<1>(sp.x), row_bc<1>(sp.y)};  // (s5, s6)
  // record for the pose / cost waves: the state BEFORE the update (the ring slot is free: see the end of the step);
  // behind the chunk's last record the publication -- which also says: this wave is done with the control records of
  // steps <= t
  if constexpr (TREE) asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(a_rec), "v"(sp.x), "n"(Q * kRecStride) : "memory");
  else asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(a_rec), "v"(sp), "n"(Q * kRecStride) : "memory");
  if constexpr (Q == 3) lds_publish(a_myseq, t + 1);
  // layer 0: [s3, s4, s5, s6, u0, u1]
  f32x2 z = {0.0f, 0.0f};
  z = __builtin_elementwise_fma(W.w1[0], f32x2{slo.x, slo.x}, z);
  z = __builtin_elementwise_fma(W.w1[1], f32x2{slo.y, slo.y}, z);
  z = __builtin_elementwise_fma(W.w1[2], f32x2{shi.x, shi.x}, z);
  z = __builtin_elementwise_fma(W.w1[3], f32x2{shi.y, shi.y}, z);
  z = __builtin_elementwise_fma(W.w1[4], f32x2{u.x, u.x}, z);
  z = __builtin_elementwise_fma(W.w1[5], f32x2{u.y, u.y}, z);
  // Requested now, used at the end of the step: (Q = 0) the control wave's count, then this rollout's controls of step
  // t+1 as ONE 8-B read into the pair the packed multiply-adds of layer 0 take them from (valid if the count read before
  // them is >= t+2).  In FRONT of layer 1: the chains below have no LDS wait of their own to hide these reads behind, and a
  // read that is still in flight when a chain starts stalls it (the packed multiply-adds formally read the odd halves of
  // the move registers, which is where the register allocator puts pending results: rollout 55.0 -> 52.4 us with the
  // reads moved here).
  int cp_v = 0;
  if constexpr (Q == 0) cp_v = *p_pub;
  if constexpr (Q == 3) pu = p_u0 + ((t + 1) & (kGRing - 1)) * kSlotF2;  // the next chunk's slots
  constexpr int kUn = (Q == 3) ? 0 : (Q + 1) * kSlotF2;
  un = pu[kUn];
  f32x2 a1 = tanh_bias2(z, W.b1s);
#pragma unroll
  for (int l = 0; l < NHH; l++) a1 = tanh_bias2(row_dot_bc(W.w2[l], a1), W.b2s[l]);  // (NHH = 0: the output layer reads layer 0)
  // Step t+1 may start when the control wave has published it (it runs ahead).  That also says that the ring slot of
  // the state record of step t+1 is free -- it held step t+1 - kGRing, consumed once cost_done >= t+2 - kGRing: the
  // control wave publishes a chunk that ends with step tm >= t+1 only after it has seen cost_done >= tm+1 - kGRing
  // (group_control_wave: need_c; the control record of a step shares the slot index of its state record), so this wave
  // does not look at the cost wave's word itself.
  // (A shorter leash for the riders -- waiting when the cost wave is more than 2 / 3 / 5 steps behind instead of a full
  // ring -- was measured: 124 / 72.6 / 58.0 us against 55.2 us; the riders need the slack.)
  // The control wave publishes whole chunks (1, 5, 9, ..., T), so the count Q = 0 has read covers the chunk's other
  // steps as a rule: they test the SGPR and read nothing.
  // The scalar side of the test in front of the output layer's chain, the (cold) wait behind it.
  const int want = t + 2;
  if constexpr (Q == 0) cp = __builtin_amdgcn_readfirstlane(cp_v);
  asm volatile("" : "+v"(un));  // the wait for the reads sits HERE (long arrived), not behind the next step's LDS stores
  if constexpr (TREE) {
    const float d = row_out_tree(W.w3, a1) + W.b3.x;
    sp.x = fmaf(d, a.dt, sp.x);  // incrementState, neural_net_model.cu:334-344
    asm volatile("" : "+v"(sp.x));
  } else {
    const f32x2 d = row_dot_bc(W.w3, a1) + W.b3;
    sp = __builtin_elementwise_fma(d, f32x2{a.dt, a.dt}, sp);  // incrementState, neural_net_model.cu:334-344
    asm volatile("" : "+v"(sp));  // the chain stays here (otherwise it is sunk below the wait, away from its moves)
  }
  if (__builtin_expect(cp < want, 0)) {  // any Q: the per-step test-and-poll, one unit of the budget per poll
    while (cp < want && --budget > 0) {
      cp = __builtin_amdgcn_readfirstlane(*p_pub);
      un = pu[kUn];
    }
    asm volatile("" : "+v"(un));  // (its wait too: otherwise the merge of the two paths puts one behind the next step's stores)
  }
}

// The dynamics wave w of a group: T - 1 network steps in aligned chunks of four, the state record of every step.
//
// Hand-over with the riders (group_roles.hpp), per CHUNK of four steps -- the riders work in chunks of four, so a word per
// step told nobody anything:
//   * xseq[w] = t0 + 4 is published once per chunk, behind the record of step t0 + 3 (and T behind the record of step
//     T - 1, which also closes a shorter last chunk).  xseq[w] >= s + 1 still means: the records of steps <= s are written,
//     and the control records of steps <= s are read (the controls of step t0 + 3 were read during step t0 + 2).
//   (a) The pose wave (and through pose_pub the cost wave) waits for the LAST record of its chunk, need = tend: it sees a
//       chunk exactly when it did with a word per step.
//   (b) The control wave tests xseq only for the reuse of a ring slot, need_x = tm - kGRing + 1 for a chunk that ends with
//       step tm = 4 m: with xseq a multiple of four that is xseq >= tm - 12, i.e. the record of step tm - 13 is out -- the
//       control wave leads the slowest dynamics wave by up to 13 steps where it led by 16.
//   (c) No cycle: the control wave publishes through step 12 without looking at xseq (need_x = 0 while tm < kGRing), which
//       lets the dynamics waves publish 4, 8, 12; from then on chunk tm needs the record of step tm - 13, which needs
//       ctl_pub >= tm - 12, published with chunk tm - 12.
//   (d) Every wait is one unit of the wave's poll budget, as before; a wave whose budget ran out (or that was started with
//       none: a.fault_wave) stops waiting, runs to its end and raises fail through spin_finish.
//   * ctl_pub is read once per chunk, by the chunk's first step in the shadow of layer 1, into an SGPR; the control wave
//     publishes 1, 5, 9, ..., T, so a count that lets step t0 + 1 start (>= t0 + 2) lets the whole chunk run.  Every step
//     still tests the SGPR (scalar compare and branch) and falls back to the poll if the count is short.
// Unrolled four times, not sixteen: two address adds per chunk remain (the record address, and the control pointer moved
// on by the chunk's last step, whose read is the only one that can wrap the ring); sixteen steps would remove them for
// four times the loop's code -- ~3 KB per chunk of the tree form.
template <int H, bool TREE, int NHH, bool GATED = false>
__device__ __forceinline__ void row_dynamics(const RolloutArgs &a, RowShared<H> &sh, const int w)
{
  static_assert(H == 32, "row_dot_bc: 32 activations, two per lane of a 16-lane row");
  static_assert(kGRing % 4 == 0, "aligned chunks of four steps inside the ring");
  const int lane = threadIdx.x & 63;
  const int r = lane >> 4, p = lane & 15;
  const int jr = 4 * w + r;  // rollout of the group
  const bool odd = (p & 1) != 0;
  const int T = a.T;
  RowWeights<H, TREE, NHH> W;
  row_load<H, TREE, NHH>(a.wpack, p, W);
  // pinned: the waits for the weight loads sit here, not at their first use inside the T loop
#pragma unroll
  for (int l = 0; l < NHH; l++)
#pragma unroll
    for (int k = 0; k < H; k++) asm volatile("" : "+v"(W.w2[l][k]));
#pragma unroll
  for (int k = 0; k < (TREE ? 4 : H); k++) asm volatile("" : "+v"(W.w3[k]));

  const uint32_t a_myseq = lds_addr(&sh.xseq[w][lane]);
  typedef const volatile int __attribute__((address_space(3))) *lds_int_p;
  typedef const volatile f32x2 __attribute__((address_space(3))) *lds_f2_p;
  const lds_int_p p_pub = (lds_int_p)&sh.ctl_pub[0];
  // clamped (u0, u1) of this lane's rollout (control wave), ring slot 0; as a finished address in a register (left as
  // base + constant the compiler re-adds the constant every time the pointer moves on)
  uint32_t a_u0 = lds_addr(&sh.ctl_rec[0][jr][0]);
  asm volatile("" : "+v"(a_u0));
  const lds_f2_p p_u = (lds_f2_p)a_u0;
  // The state record of a step is stored by EVERY lane: lanes 0, 1 of a row into the record, the others into a dump row
  // nobody reads -- no exec masking on the recurrence; both move along with the ring slot (one address add for all lanes).
  // (tree form: one component per lane -- quad q of the row holds s[3 + q], lanes 0, 4, 8, 12 write the record)
  const uint32_t a_rec0 = TREE ? (((p & 3) == 0) ? lds_addr(&sh.rec[0][jr][p >> 2]) : lds_addr(&sh.dump[w][2 * lane]))
                               : ((p < 2) ? lds_addr(&sh.rec[0][jr][2 * p]) : lds_addr(&sh.dump[w][2 * lane]));
  constexpr uint32_t kRecStride = sizeof(float) * kRolloutsPerWave * 4;

  // this lane's pair of the state: (s3, s4) for even p, (s5, s6) for odd p -- every even / odd lane of a rollout computes
  // the same output pair; layer 0 takes the pairs of lanes 0 and 1 of the row
  // (tree form: sp.x = s[3 + (p >> 2)], sp.y unused)
  int budget = spin_budget_init(a.spin_budget, T, a.fault_wave == w + 1);
  f32x2 sp;
  if constexpr (GATED) {
    // the state arrives through the gate block: the pose wave has put it into LDS (the weights above were loaded meanwhile)
    const uint32_t a_go = lds_addr(&sh.gate_open[0]);
    while (lds_peek(a_go) == 0 && --budget > 0) __builtin_amdgcn_s_sleep(1);
    const volatile float *gs = sh.gstate;
    sp = TREE ? f32x2{gs[3 + (p >> 2)], 0.0f} : odd ? f32x2{gs[5], gs[6]} : f32x2{gs[3], gs[4]};
  } else {
    sp = TREE ? f32x2{a.state[3 + (p >> 2)], 0.0f} : odd ? f32x2{a.state[5], a.state[6]} : f32x2{a.state[3], a.state[4]};
  }
  if (w == 0) RSTAMP(2);  // weights in registers
  int cp = 0;  // steps the control wave has published, as far as this wave knows (SGPR)
  while ((cp = __builtin_amdgcn_readfirstlane(*p_pub)) < 1 && --budget > 0) __builtin_amdgcn_s_sleep(1);
  if (w == 0) RSTAMP(3);  // first controls published: the T loop starts
  lds_f2_p pu = p_u;  // the control records of the chunk: slot t0 % kGRing
  f32x2 un = pu[0];
  asm volatile("" : "+v"(un));  // pinned: the wait for this read sits here, not inside the loop

  // Steps 0 .. T-2 in full; of step T-1 only the state record goes out (its update feeds nothing: the cost is the
  // running mean over the states BEFORE the updates of steps 1..T-1, mppi_controller.cu:160-177).  One copy of the step
  // per position of the chunk; a last chunk of fewer steps leaves it early.
  const int NS = T - 1;
  for (int t0 = 0; t0 < NS; t0 += 4) {
    const uint32_t a_rec = a_rec0 + (uint32_t)(t0 & (kGRing - 1)) * kRecStride;
    row_step<H, TREE, NHH, 0>(a, W, sp, un, t0, a_rec, a_myseq, p_pub, pu, p_u, cp, budget);
    if (t0 + 1 >= NS) break;
    row_step<H, TREE, NHH, 1>(a, W, sp, un, t0, a_rec, a_myseq, p_pub, pu, p_u, cp, budget);
    if (t0 + 2 >= NS) break;
    row_step<H, TREE, NHH, 2>(a, W, sp, un, t0, a_rec, a_myseq, p_pub, pu, p_u, cp, budget);
    if (t0 + 3 >= NS) break;
    row_step<H, TREE, NHH, 3>(a, W, sp, un, t0, a_rec, a_myseq, p_pub, pu, p_u, cp, budget);
  }
  if (w == 0) RSTAMP(4);  // T loop done
  {  // the record of step T-1, and the publication that closes the last chunk
    const int t = T - 1;
    if constexpr (TREE) asm volatile("ds_write_b32 %0, %1" ::"v"(a_rec0 + (uint32_t)(t & (kGRing - 1)) * kRecStride), "v"(sp.x) : "memory");
    else asm volatile("ds_write_b64 %0, %1" ::"v"(a_rec0 + (uint32_t)(t & (kGRing - 1)) * kRecStride), "v"(sp) : "memory");
    lds_publish(a_myseq, t + 1);
  }
  spin_finish(budget, lds_addr(&sh.fail[0]), lds_addr(&sh.fin[w]));
}

// one group (workgroup): the four dynamics waves and the four riders
template <int H, int NHH, bool AFFINE, bool CTRL, bool TREE, bool GATED = false>
__device__ __forceinline__ void row_group(const RolloutArgs &a, RowShared<H> &sh)
{
  using SH = RowShared<H>;
  using R = GroupRoles<SH>;
  const int lane = threadIdx.x & 63;
  const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (role == 0) RSTAMP(0);  // first instruction
  MrgHalf g0{0, 0, 0};
  if (role == R::kRng) g0 = group_rng_load<SH>(a);  // in front of the barrier: the head of the launch's critical path
  if (role == 0) {  // sequence words start at 0; the only barrier
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
  __syncthreads();
  if (role == 0) RSTAMP(1);  // behind the barrier
#ifdef MPPI_ROW_RIDER_PRIO
  if (role >= 4) __builtin_amdgcn_s_setprio(MPPI_ROW_RIDER_PRIO);
#endif
  if (role < 4) row_dynamics<H, TREE, NHH, GATED>(a, sh, role);
  else if (role == R::kCost) { group_cost_wave4<SH, CTRL>(a, sh); RSTAMP(5); }  // costs stored
  else if (role == R::kCtl) { group_control_wave(a, sh, GATED ? lds_addr(&sh.gate_open[0]) : 0u); RSTAMP(6); }
  else if (role == R::kPose) {
    if constexpr (GATED) {
      const int shut = group_gate_wait(a, sh);
      const volatile float *gs = sh.gstate;
      const float x0 = gs[0], y0 = gs[1], yaw0 = gs[2];
      group_pose_wave4<SH, AFFINE>(a, sh, x0, y0, yaw0, shut);
    } else {
      group_pose_wave4<SH, AFFINE>(a, sh);
    }
    RSTAMP(7);
  }
  else { group_rng_wave<SH, true>(a, sh, g0); RSTAMP(8); }
}

}  // namespace mppi
