// abi_forms.hip -- which rollout kernel form serves a handle: the selection TABLE (model shape x rollout groups per CU ->
// form, every row with the measurement that justifies it), the descriptor table kForms (what the host knows about a form: image,
// noise source, launch adapters, name), the table of request names kRequests behind mppi_set_rollout_variant.
// tests/test_form_selection_gpu.py times the candidates of every bucket and fails if the table's choice is more than
// 10 % slower than the best of them.
#include "abi_internal.hpp"

using namespace mppi;
using namespace mppi_abi;

namespace mppi_abi {

bool use_mfma(const mppi_handle *h)
{
  if (h->basis || h->pref == Pref::Valu || h->pref == Pref::ValuLds) return false;
  return h->mfma_ok;
}

// "valu" on a standard shape runs the register/scalar-operand kernel; "valu_lds" forces the generic one
bool use_valu_reg(const mppi_handle *h) { return !h->basis && !use_mfma(h) && h->valu_reg_ok && h->pref != Pref::ValuLds; }

namespace {

// The network model on a 6 -> hidden x n_hidden -> 4 shape: first row that matches the shape (0 = any), serves the
// handle's 16-rollout groups per CU (0 = any number), exists for the shape and -- when "mfma" asked for the reference's
// summation order (the A/B arm of SURVEY cfg 4) -- keeps that order.  MI355X: 256 CUs of 4 SIMDs; times are rollout-kernel
// times at T = 100 unless a row says otherwise.
struct FormRule {
  int hidden, n_hidden, max_groups_per_cu;
  Form form;
  bool exact;  // the reference's k-ascending sums in every layer: bit-identical to every other exact form
  const char *evidence;
};
const FormRule kFormRules[] = {
    // 64-wide nets in the latency regime: v_mfma_f32_4x4x1 with A-broadcast, every hidden weight in registers, no hand-over
    // between waves (rollout_m44.hip); output layer as a butterfly and -- since the end of round 4 -- the hidden layers as two
    // accumulation chains (K=1920 6-64x4-4 148.5 -> 119.0 us, K=4096 6-64-64-4 70.3 -> 60.6 us, profiles/r04_x_m44_split_ab.txt),
    // inside the north-star tolerance (tests/test_m44_gpu.py); "m44_chain" keeps the reference's order in the hidden layers
    {64, 2, 2, Form::M44, false, "profiles/r04_d_m44_first.txt: K=4096 70.5 us (oct 101, row64 107); K=8192 128 us (oct 166): 110 VGPRs, two workgroups per CU"},
    {64, 4, 2, Form::M44, false, "profiles/r04_d_m44_first.txt: 6-64x4-4 K=1920 149 us (oct 181, row64 227); K=4096 150 us (oct 182); 240 VGPRs = one workgroup per CU, so K=8192 runs in two rounds and still leads: T=60 182 us (oct 217), profiles/r04_e_form_selection.txt"},
    // ... in the reference's order: one M tile per dynamics wave, four of them + four riders (rollout_oct.hip)
    {64, 0, 2, Form::Oct, true, "K=4096: 6-64-64-4 oct 108 us, quad 134; 6-64x4-4 oct 185, quad 279; K=8192: oct 172, multi2 187; 6-64x4-4 oct 365, fused 503; at four groups per CU it loses, 724 vs 508 (profiles/r03_i_*)"},
    // 6-32-32-4 at one group per CU: the recurrence on the vector ALU (rollout_row.hip), output layer as a butterfly
    {32, 2, 2, Form::RowTree, false, "profiles/r04_a_headline_row_tree_*: K=4096 36.7 us (row_exact 45.8, quad 68.0); two groups per CU (106 VGPRs): K=8192 60.3 us (multi2 78.0, multi4 84.2), profiles/r04_e_form_selection.txt; tests/test_row_tree_gpu.py, profiles/r04_b_fuzz_sweep_row_tree_10639_draws.txt"},
    // up to one group per CU: the network split over two SIMDs + a cost and a control wave (rollout_mfma.hip, quad form)
    {0, 0, 1, Form::Quad, true, "6-32-32-4 K=4096: quad 71 us, multi1 / multi2 83, single-wave 122 (profiles/r02_*); row_exact 45.8 is not bit-for-bit needed when \"mfma\" is asked for"},
    // up to two: two dynamics waves (whole network each) + cost + control wave, every wave on a SIMD of its own
    {0, 0, 2, Form::Multi2, true, "K=8192: multi2 77-83 us, quad 112, single-wave 123, row at two groups per CU 93; 6-64-64-4 T=150: 277 vs 359 / 339 us"},
    // beyond: four dynamics waves per workgroup, one per SIMD, riders on the side, eps from the stand-alone generator kernel;
    // the output layer -- 8 of 28 / 16 of 88 matrix instructions per step for 4 useful rows of a 16-row tile -- as a butterfly
    // over the four lanes of a rollout (mfma_net.hpp: nn_last_tree; inside the north-star tolerance, tests/test_multi_tree_gpu.py)
    {0, 0, 0, Form::Multi4Tree, false, "profiles/r04_l_multi4_tree.txt"},
    {0, 0, 0, Form::Multi4, true, "K=16384: 87.5 us (profiles/r03_i_k16384_*) vs 124 single-wave; 6-64-64-4 T=150: 271 us (profiles/r03_d_cfg4_*) vs 341; the in-kernel generator would load one SIMD too much: 341 us"},
    // shapes the multi form does not have (6-64x4-4 beyond two groups per CU): one wave per 16 rollouts does everything, in
    // workgroups of FOUR waves -- the dispatcher spreads a workgroup's waves over the four SIMDs of a CU, whereas 64-thread
    // workgroups are placed one by one and sometimes two on one SIMD (tools/placement_probe.hip: rollout 601 vs 341 us)
    {0, 0, 0, Form::Fused256, true, "6-64x4-4 K=16384: 508 us vs oct 724"},
};

}  // namespace

// The descriptor table: everything the host knows about a form outside the selection policy above.  First the launch adapters:
// they pass on what a kernel's launcher takes beside the argument block (d.arg: the row's own integer).
namespace {
hipError_t one_mfma(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_mfma(h->hidden, h->n_hidden, a, d.arg, s); }    // arg: threads per workgroup
hipError_t one_multi(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_multi(h->hidden, h->n_hidden, a, d.arg, s); }  // arg: ND; 44 = ND 4 with the tree output layer
hipError_t one_oct(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_oct(h->hidden, h->n_hidden, a, s); }
hipError_t one_row(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_row(h->hidden, h->n_hidden, a, d.arg != 0, s); }  // arg: tree
hipError_t one_row64(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_row64(h->hidden, h->n_hidden, a, d.arg, s); }   // arg: rollouts per group
hipError_t one_m44(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_m44(h->hidden, h->n_hidden, a, d.arg != 0, s); }  // arg: split
hipError_t one_lds44(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_lds44(h->net, a, s); }
hipError_t one_lds128(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_lds128(h->net, a, s); }
hipError_t one_lds16(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_lds16(h->net, a, h->num_simds / 4, s); }
hipError_t one_glb16(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_glb16(h->net, a, h->num_simds / 4, h->glb16_cap, s); }
hipError_t one_glb44(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_glb44(h->net, a, h->glb44_cap, s); }
hipError_t one_row32(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_row32(h->net, a, d.arg != 0, s); }  // arg: tree
hipError_t one_fleet(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_fleet_one(h, a); }  // the fleet's kernel with one instance, on the handle's own stream
hipError_t one_valu_reg(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_valu_reg(h->hidden, h->n_hidden, a, s); }
hipError_t one_valu(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_valu(h->net, a, s); }
hipError_t one_bf(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_bf(a, d.arg, s); }  // arg: waves per 64 rollouts
hipError_t one_bf_row(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t s) { return launch_rollout_bf_row(a, s); }
hipError_t batch_quad(const mppi_handle *h0, const FormDesc &d, const QuadBatchArgs &qb, hipStream_t s) { return launch_rollout_quad_batch(h0->hidden, h0->n_hidden, qb, s); }
hipError_t batch_row(const mppi_handle *h0, const FormDesc &d, const QuadBatchArgs &qb, hipStream_t s) { return launch_rollout_row_batch(qb, d.arg != 0, s); }
hipError_t batch_m44(const mppi_handle *h0, const FormDesc &d, const QuadBatchArgs &qb, hipStream_t s) { return launch_rollout_m44_batch(h0->n_hidden, qb, s); }
hipError_t batch_lds44(const mppi_handle *h0, const FormDesc &d, const QuadBatchArgs &qb, hipStream_t s) { return launch_rollout_lds44_batch(h0->net, qb, s); }
hipError_t batch_lds128(const mppi_handle *h0, const FormDesc &d, const QuadBatchArgs &qb, hipStream_t s) { return launch_rollout_lds128_batch(h0->net, qb, s); }
hipError_t batch_glb44(const mppi_handle *h0, const FormDesc &d, const QuadBatchArgs &qb, hipStream_t s) { return launch_rollout_glb44_batch(h0->net, qb, h0->glb44_cap, s); }
hipError_t batch_row32(const mppi_handle *h0, const FormDesc &d, const QuadBatchArgs &qb, hipStream_t s) { return launch_rollout_row32_batch(h0->net, qb, d.arg != 0, s); }
hipError_t batch_bf(const mppi_handle *h0, const FormDesc &d, const QuadBatchArgs &qb, hipStream_t s) { return launch_rollout_bf_batch(qb, s); }
hipError_t batch_bf_row(const mppi_handle *h0, const FormDesc &d, const QuadBatchArgs &qb, hipStream_t s) { return launch_rollout_bf_row_batch(qb, s); }
// the fleet adapters: the forms of one list / shape / wave count read it from the first handle (fleet_together: it is every handle's)
hipError_t fleet_16(mppi_handle *const *hs, const RolloutArgs *h_inst, const RolloutArgs *d_inst, const FleetGlbNet *, int n, hipStream_t s) { return launch_rollout_fleet16(hs[0]->net, h_inst, d_inst, n, hs[0]->num_simds / 4, s); }
hipError_t fleet_multi(mppi_handle *const *hs, const RolloutArgs *h_inst, const RolloutArgs *d_inst, const FleetGlbNet *, int n, hipStream_t s) { return launch_rollout_fleet_multi(hs[0]->hidden, hs[0]->n_hidden, h_inst, d_inst, n, s); }
hipError_t fleet_bf(mppi_handle *const *hs, const RolloutArgs *h_inst, const RolloutArgs *d_inst, const FleetGlbNet *, int n, hipStream_t s) { return launch_rollout_fleet_bf(h_inst, d_inst, n, hs[0]->num_simds, hs[0]->fleet_bf_waves, s); }
// every handle's own list and cap
hipError_t fleet_glb16(mppi_handle *const *hs, const RolloutArgs *h_inst, const RolloutArgs *d_inst, const FleetGlbNet *d_nets, int n, hipStream_t s)
{
  if (n < 1 || n > kMaxFleet) return hipErrorInvalidValue;
  NetDesc nets[kMaxFleet];
  int caps[kMaxFleet];
  for (int i = 0; i < n; i++) {
    nets[i] = hs[i]->net;
    caps[i] = hs[i]->glb16_cap;
  }
  return launch_rollout_fleet_glb16(nets, caps, h_inst, d_inst, d_nets, n, hs[0]->num_simds / 4, s);
}
FleetGlbNet fleet_glb16_net(const mppi_handle *h) { return fleet_glb16_net_of(h->net, h->glb16_cap); }
constexpr const char *kMfma16 = "mfma16x16x4", *kMfma4 = "mfma4x4x1";
constexpr FormDesc kForms[] = {
    // form, image, noise, flags, standard shapes, launch, arg, batch {launch, pair only, same list, waves}, fleet, cap, name {stem, tag, suffix, gen}, ask {first, second, K multiple}[, fleet net]
    {Form::Auto, Image::Mfma, Noise::Never, 0, nullptr, nullptr, 0, {}, nullptr, nullptr, {""}, {}},  // form_of never answers Auto
    {Form::Fused64, Image::Mfma, Noise::Never, 0, mfma_variant_supported, one_mfma, 64, {}, nullptr, nullptr, {kMfma16, Tag::HiddenLayers, "_fused_b64"}, {}},
    {Form::Fused256, Image::Mfma, Noise::Never, 0, mfma_variant_supported, one_mfma, 256, {}, nullptr, nullptr, {kMfma16, Tag::HiddenLayers, "_fused_b256"}, {"fused"}},
    {Form::Quad, Image::Mfma, Noise::InKernel, 0, mfma_variant_supported, one_mfma, 512, {batch_quad, false, false, 16}, nullptr, nullptr, {kMfma16, Tag::HiddenLayers, "_quad4w"}, {"quad"}},
    {Form::Oct, Image::Mfma, Noise::UnlessStandalone, 0, oct_variant_supported, one_oct, 0, {}, nullptr, nullptr, {kMfma16, Tag::HiddenLayers, "_oct8w", true}, {"oct"}},
    {Form::Multi2, Image::Mfma, Noise::UnlessStandalone, kPublishes, multi_variant_supported, one_multi, 2, {}, nullptr, nullptr, {kMfma16, Tag::HiddenLayers, "_multi2", true}, {"multi2", nullptr, 32}},
    {Form::Multi4, Image::Mfma, Noise::UnlessStandalone, kPublishes, multi_variant_supported, one_multi, 4, {}, nullptr, nullptr, {kMfma16, Tag::HiddenLayers, "_multi4", true}, {"multi4_gen", nullptr, 64}},
    {Form::Multi4Tree, Image::Mfma, Noise::UnlessStandalone, kPublishes, multi_variant_supported, one_multi, 44, {}, nullptr, nullptr, {kMfma16, Tag::HiddenLayers, "_multi4_tree", true}, {"multi4_tree_gen", nullptr, 64}},
    {Form::Row, Image::Row, Noise::InKernel, kGate, row_variant_supported, one_row, 0, {batch_row, false, false, 16}, nullptr, nullptr, {"valu_row8w", Tag::HiddenLayers}, {}},
    {Form::RowTree, Image::Row, Noise::InKernel, kGate, row_variant_supported, one_row, 1, {batch_row, false, false, 16}, nullptr, nullptr, {"valu_row8w_tree", Tag::HiddenLayers}, {"row_tree", "row_exact"}},
    {Form::Row64R16, Image::Row64, Noise::InKernel, 0, row64_variant_supported, one_row64, 16, {}, nullptr, nullptr, {"valu_row64_r16_tree", Tag::HiddenLayers}, {}},
    {Form::M44, Image::M44, Noise::InKernel, kGate, m44_variant_supported, one_m44, 1, {batch_m44, true, false, 16}, nullptr, nullptr, {kMfma4, Tag::HiddenLayers, "_m44_split_tree"}, {"m44", "m44_chain"}},
    {Form::M44Chain, Image::M44, Noise::InKernel, 0, m44_variant_supported, one_m44, 0, {}, nullptr, nullptr, {kMfma4, Tag::HiddenLayers, "_m44_tree"}, {}},
    {Form::Lds44, Image::Lds44, Noise::InKernel, kGate | kByName, nullptr, one_lds44, 0, {batch_lds44, true, true, 16}, nullptr, nullptr, {"mfma4x4x1_lds", Tag::LayersWidth}, {}},
    {Form::Lds128, Image::Lds128, Noise::InKernel, kGate | kByName, nullptr, one_lds128, 0, {batch_lds128, true, true, 16}, nullptr, nullptr, {"mfma4x4x1_lds2h", Tag::LayersWidth}, {}},
    {Form::Lds16, Image::Lds16, Noise::Never, kByName, nullptr, one_lds16, 0, {}, nullptr, nullptr, {"mfma16x16x4_lds", Tag::LayersWidth}, {}},
    {Form::Glb16, Image::Glb16, Noise::Never, kByName, nullptr, one_glb16, 0, {}, nullptr, &mppi_handle::glb16_cap, {"mfma16x16x4_glb", Tag::LayersWidth}, {}},
    {Form::Glb44, Image::Glb44, Noise::InKernel, kGate | kByName, nullptr, one_glb44, 0, {batch_glb44, true, true, 16}, nullptr, &mppi_handle::glb44_cap, {"mfma4x4x1_glb", Tag::LayersWidth}, {}},
    {Form::Fleet16, Image::Lds16, Noise::Never, kByName, nullptr, one_fleet, 0, {}, fleet_16, nullptr, {"mfma16x16x4_fleet", Tag::LayersWidth}, {}},
    {Form::FleetMulti4, Image::Mfma, Noise::Never, kPublishes | kByName, multi_variant_supported, one_fleet, 0, {}, fleet_multi, nullptr, {kMfma16, Tag::HiddenLayers, "_fleet_multi4_tree", true}, {}},
    {Form::FleetGlb16, Image::Glb16, Noise::Never, kByName, nullptr, one_fleet, 0, {}, fleet_glb16, &mppi_handle::glb16_cap, {"mfma16x16x4_fleet_glb", Tag::LayersWidth}, {}, fleet_glb16_net},
    {Form::ValuReg, Image::ThetaS, Noise::Never, 0, nullptr, one_valu_reg, 0, {}, nullptr, nullptr, {"valu_reg_lds"}, {}},
    {Form::ValuLds, Image::Theta, Noise::Never, 0, nullptr, one_valu, 0, {}, nullptr, nullptr, {"valu_lds"}, {}},
    {Form::Bf1, Image::Theta, Noise::Never, 0, nullptr, one_bf, 1, {}, nullptr, nullptr, {"basis_funcs25_valu"}, {}},
    {Form::Bf2, Image::Theta, Noise::Never, 0, nullptr, one_bf, 2, {}, nullptr, nullptr, {"basis_funcs25_valu_2w"}, {}},
    {Form::Bf3, Image::Theta, Noise::InKernel, 0, nullptr, one_bf, 3, {batch_bf, false, false, 3}, nullptr, nullptr, {"basis_funcs25_valu_3w"}, {}},
    {Form::BfRow, Image::BfRow, Noise::InKernel, kGate | kByName | kNegateYaw, nullptr, one_bf_row, 0, {batch_bf_row, true, false, 16}, nullptr, nullptr, {"basis_funcs25_row8w"}, {}},
    {Form::Row32, Image::Row32, Noise::InKernel, kGate | kByName, nullptr, one_row32, 0, {batch_row32, true, true, 16}, nullptr, nullptr, {"valu_row8w", Tag::LayersWidth}, {}},
    {Form::Row32Tree, Image::Row32, Noise::InKernel, kGate | kByName, nullptr, one_row32, 1, {batch_row32, true, true, 16}, nullptr, nullptr, {"valu_row8w_tree", Tag::LayersWidth}, {}},
    {Form::FleetBf, Image::Theta, Noise::Never, kByName, nullptr, one_fleet, 0, {}, fleet_bf, nullptr, {"basis_funcs25_fleet", Tag::ForcedWaves}, {}},
};
static_assert(rows_in_order(kForms, &FormDesc::form), "row i of kForms describes form i");
}  // namespace
const FormDesc &form_desc(Form f) { return kForms[(int)f]; }
static bool form_supported(Form f, int hidden, int n_hidden) { return kForms[(int)f].shape && kForms[(int)f].shape(hidden, n_hidden); }

Form form_of(const mppi_handle *h)
{
  if (h->basis) {
    // basis-function model, wavefronts per 64 rollouts: dynamics + cost + control wave (in-kernel generator) while each gets
    // a SIMD of its own; dynamics + cost wave up to twice that; else one wave
    if (h->forced == Form::Bf1 || h->forced == Form::Bf2 || h->forced == Form::Bf3) return h->forced;
    if (h->forced == Form::BfRow || h->forced == Form::FleetBf) return h->forced;  // by name only
    if (3 * (h->K / 64) <= h->num_simds) return Form::Bf3;
    return (2 * (h->K / 64) <= 2 * h->num_simds) ? Form::Bf2 : Form::Bf1;
  }
  if (form_desc(h->forced).has(kByName)) return h->forced;
  if (!use_mfma(h)) return use_valu_reg(h) ? Form::ValuReg : Form::ValuLds;
  if (h->forced != Form::Auto) return h->forced;
  const int groups = h->K / kRolloutsPerWave, cus = h->num_simds / 4;
  for (const FormRule &r : kFormRules) {
    if ((r.hidden != 0 && r.hidden != h->hidden) || (r.n_hidden != 0 && r.n_hidden != h->n_hidden)) continue;
    if (r.max_groups_per_cu != 0 && groups > r.max_groups_per_cu * cus) continue;
    if (!form_supported(r.form, h->hidden, h->n_hidden)) continue;
    if (h->pref == Pref::Mfma && !r.exact) continue;
    return r.form;
  }
  return Form::Fused256;
}

// oct / multi forms: eps from the stand-alone generator kernel (forced by "_gen", and the automatic choice for ND = 4)
bool form_generator_noise(const mppi_handle *h)
{
  if (h->forced != Form::Auto) return h->multi_standalone_noise;
  const Form f = form_of(h);
  return f == Form::Multi4 || f == Form::Multi4Tree;
}

// does the rollout kernel draw eps itself (a control / noise wavefront with the in-kernel MRG32k3a)?
bool has_noise_wave(const mppi_handle *h)
{
  const Noise n = form_desc(form_of(h)).noise;
  return n == Noise::InKernel || (n == Noise::UnlessStandalone && !form_generator_noise(h));
}

}  // namespace mppi_abi

static int widest_hidden(const NetDesc &net)
{
  int wmax = 0;
  for (int l = 1; l + 1 < net.n_layers; l++) wmax = std::max(wmax, net.layers[l]);
  return wmax;
}

// the cap of "<form>_r<N>" (suffix = what follows the form's name): -1 for no suffix, -2 for anything else ("unknown variant")
static int resident_cap_of(const char *suffix)
{
  if (*suffix == 0) return -1;
  const char *p = suffix + 2;
  if (strncmp(suffix, "_r", 2) != 0 || *p == 0 || strlen(p) > 9) return -2;
  for (const char *q = p; *q; q++)
    if (*q < '0' || *q > '9') return -2;
  return atoi(p);
}

// The request names of mppi_set_rollout_variant.  A request is refused by the first of its preconditions that does not hold, in the
// order of the columns: model kind, shape (and its second limit, the last column), K multiple, LDS limit, image present, preparation step.  (Every K multiple divides 64
// and mppi_create refuses a K that 64 does not divide: that check is a guard no caller can see, whatever its place.)
namespace {
using Shape = bool (*)(const mppi_handle *h, Form f);  // f: the form the request would force
bool table_shape(const mppi_handle *h, Form) { return h->mfma_ok; }
bool form_shape(const mppi_handle *h, Form f) { return h->mfma_ok && form_supported(f, h->hidden, h->n_hidden); }
bool lds44_shape(const mppi_handle *h, Form) { return lds44_supported(h->net); }
bool lds128_shape(const mppi_handle *h, Form) { return lds128_lds_bytes(h->net) != 0; }
bool lds16_shape(const mppi_handle *h, Form) { return lds16_lds_bytes(h->net) != 0; }
bool glb16_shape(const mppi_handle *h, Form) { return glb16_supported(h->net); }
bool glb44_shape(const mppi_handle *h, Form) { return glb44_supported(h->net); }
bool row32_shape(const mppi_handle *h, Form) { return row32_supported(h->net, true); }
bool row32_exact_depth(const mppi_handle *h, Form) { return row32_supported(h->net, false); }
// the image of a form built on request; without parameters yet: mppi_set_nn_params builds it
int build_image(mppi_handle *h, Form f)
{
  const Image id = form_desc(f).image;
  return (!image(h, id) && h->have_nn) ? upload_image(h, id) : MPPI_OK;
}
int prepare_fleet(mppi_handle *h, Form) { return fleet_prepare(h, false); }
// glb16's image (built at this call) and the handle's own argument block with its layer-list descriptor
int prepare_fleet_glb16(mppi_handle *h, Form f)
{
  if (int rc = build_image(h, f)) return rc;
  return fleet_prepare(h, true);
}

enum class Model { Any, Network, Basis };
enum class Gen { Keep, Off, On };  // multi_standalone_noise: eps from the stand-alone generator ("_gen")
struct Request {
  const char *name;         // the spelling; with_cap: "<name>" or "<name>_r<N>" (at most N blocks / quads of the stream resident)
  bool with_cap;
  Form net, bf;             // the form it forces on the network model / on the basis-function model
  int pref;                 // >= 0: the request is a preference (Pref), and a form forced earlier does not stick
  Gen gen;
  Model model;              // refusal: "<name> is a form of the ... model"
  Shape shape;              // nullptr: any
  const char *shape_msg;
  int k_multiple;           // with k_msg
  const char *k_msg;
  size_t (*lds_bytes)(const NetDesc &net);  // the LDS the weights of the list need per <lds_unit>, held against lds_limit()
  size_t (*lds_limit)();
  const char *lds_unit;
  bool needs_image;         // the form's image was allocated with the handle; refusal: "<name> form: this handle has no image"
  int (*prepare)(mppi_handle *h, Form f);
  int waves;                // "fleet_bf_w<N>": the wave count the request forces on the fleet's launch; 0: none
  const char *say;          // the name its refusals speak of; nullptr: its own
  Shape shape2;             // a second limit on the shape, checked behind `shape`, with its own refusal; nullptr: none
  const char *shape2_msg;
};
const char kRowMsg[] = "row form exists for 6-32x2-4", kM44Msg[] = "m44 form exists for 6-64x2-4 and 6-64x4-4",
           kRow64Msg[] = "row64 form exists for 6-64x2-4 and 6-64x4-4", kOctMsg[] = "oct form exists for 6-64x2-4 and 6-64x4-4",
           kMultiMsg[] = "multi form exists for 6-32x2-4, 6-32x4-4 and 6-64x2-4", kMultiK[] = "multi form needs K to be a multiple of 16 ND",
           kLds128Msg[] = "lds128 form needs 6 -> hidden widths 1..128 -> 4 with at least one hidden layer",
           kLds16Msg[] = "lds16 form needs 6 -> hidden widths 1..128 -> 4 with at least one hidden layer",
           kGlb16Msg[] = "glb16 form needs 6 -> hidden widths 1..256 -> 4 with at least one hidden layer",
           kGlb44Msg[] = "glb44 form needs 6 -> hidden widths 1..256 -> 4 with at least one hidden layer",
           kRow32Msg[] = "row32 form needs 6 -> one to four hidden widths 1..32 -> 4",
           kRow32TreeMsg[] = "row32_tree form needs 6 -> one to four hidden widths 1..32 -> 4",
           kRow32DepthMsg[] = "row32 form keeps the reference's order for at most three hidden layers: the fourth does not fit the registers (row32_tree serves four)",
           kFleetBfK[] = "fleet_bf form needs K to be a multiple of 64";
constexpr int kNoPref = -1;
const Request kRequests[] = {
    // name, with cap, network form, basis form, pref, gen | model, shape, its refusal | K multiple | LDS bytes, limit, unit | image | preparation
    {"auto", false, Form::Auto, Form::Auto, (int)Pref::Auto, Gen::Keep},
    // the table again, restricted to the forms in the reference's order
    {"mfma", false, Form::Auto, Form::Auto, (int)Pref::Mfma, Gen::Keep, Model::Any, table_shape, "MFMA variant needs 6-HxN-4 with H in {32,64}, N in {2,4}"},
    {"valu", false, Form::Auto, Form::Auto, (int)Pref::Valu, Gen::Keep},
    {"valu_lds", false, Form::Auto, Form::Auto, (int)Pref::ValuLds, Gen::Keep},
    {"quad", false, Form::Quad, Form::Bf2, kNoPref, Gen::Keep},
    {"bf3", false, Form::Bf3, Form::Bf3, kNoPref, Gen::Keep, Model::Basis},
    // the latency form of the basis-function model; the bits of bf3
    {"bf_row", false, Form::BfRow, Form::BfRow, kNoPref, Gen::Keep, Model::Basis, nullptr, nullptr, kRolloutsPerWave, "bf_row form needs K to be a multiple of 16", nullptr, nullptr, nullptr, true},
    {"row", false, Form::Row, Form::Row, kNoPref, Gen::Keep, Model::Any, form_shape, kRowMsg},
    {"row_exact", false, Form::Row, Form::Row, kNoPref, Gen::Keep, Model::Any, form_shape, kRowMsg},
    {"row_tree", false, Form::RowTree, Form::RowTree, kNoPref, Gen::Keep, Model::Any, form_shape, kRowMsg},
    {"m44", false, Form::M44, Form::M44, kNoPref, Gen::Keep, Model::Any, form_shape, kM44Msg},
    {"m44_chain", false, Form::M44Chain, Form::M44Chain, kNoPref, Gen::Keep, Model::Any, form_shape, kM44Msg},
    // any layer list up to 64 wide; the reference's order in every layer
    {"lds44", false, Form::Lds44, Form::Lds44, kNoPref, Gen::Keep, Model::Network, lds44_shape,
     "lds44 form needs 6 -> hidden widths 1..64 -> 4 with at least one hidden layer"},
    // any layer list up to 128 wide whose image fits one workgroup's LDS: the latency form, the throughput form
    {"lds128", false, Form::Lds128, Form::Lds128, kNoPref, Gen::Keep, Model::Network, lds128_shape, kLds128Msg, 1, nullptr,
     lds128_lds_bytes, lds128_lds_limit, "group", true},
    {"lds16", false, Form::Lds16, Form::Lds16, kNoPref, Gen::Keep, Model::Network, lds16_shape, kLds16Msg, 1, nullptr,
     lds16_lds_bytes, lds16_lds_limit, "workgroup", true},
    // lds16's wave, image and lists; up to 64 such handles share the launches of a batched solve
    {"fleet16", false, Form::Fleet16, Form::Fleet16, kNoPref, Gen::Keep, Model::Network, lds16_shape,
     "fleet16 form needs 6 -> hidden widths 1..128 -> 4 with at least one hidden layer", 1, nullptr, lds16_lds_bytes, lds16_lds_limit,
     "workgroup", true, prepare_fleet},
    // "multi4_tree_gen"'s workgroup and bits (eps from the stand-alone generator: no form with the in-kernel one); up to 64 such
    // handles share the launches of a batched solve
    {"fleet_multi4", false, Form::FleetMulti4, Form::FleetMulti4, kNoPref, Gen::On, Model::Network, form_shape,
     "fleet_multi4 form exists for 6-32x2-4, 6-32x4-4 and 6-64x2-4", 64, "fleet_multi4 form needs K to be a multiple of 64", nullptr, nullptr, nullptr, false, prepare_fleet},
    // the workgroups of the basis-function model's own kernels and the bits of "bf3" (eps from the stand-alone generator); up to 64
    // such handles share the launches of a batched solve.  "fleet_bf": the wave count per 64 rollouts is fleet_bf_plan's choice;
    // "_w1" / "_w2" / "_w3": that count forced (tests and A/Bs: every kernel at any shape on any device)
    {"fleet_bf", false, Form::FleetBf, Form::FleetBf, kNoPref, Gen::On, Model::Basis, nullptr, nullptr, 64, kFleetBfK, nullptr, nullptr, nullptr, false, prepare_fleet},
    {"fleet_bf_w1", false, Form::FleetBf, Form::FleetBf, kNoPref, Gen::On, Model::Basis, nullptr, nullptr, 64, kFleetBfK, nullptr, nullptr, nullptr, false, prepare_fleet, 1, "fleet_bf"},
    {"fleet_bf_w2", false, Form::FleetBf, Form::FleetBf, kNoPref, Gen::On, Model::Basis, nullptr, nullptr, 64, kFleetBfK, nullptr, nullptr, nullptr, false, prepare_fleet, 2, "fleet_bf"},
    {"fleet_bf_w3", false, Form::FleetBf, Form::FleetBf, kNoPref, Gen::On, Model::Basis, nullptr, nullptr, 64, kFleetBfK, nullptr, nullptr, nullptr, false, prepare_fleet, 3, "fleet_bf"},
    // lds16's wave / lds128's group for every layer list up to 256 wide
    {"glb16", true, Form::Glb16, Form::Glb16, kNoPref, Gen::Keep, Model::Network, glb16_shape, kGlb16Msg, 64, "glb16 form needs K to be a multiple of 64", nullptr,
     nullptr, nullptr, false, build_image},
    // glb16's wave, image and lists; up to 64 such handles, every one with its own list and cap, share the launches of a batched solve
    {"fleet_glb16", true, Form::FleetGlb16, Form::FleetGlb16, kNoPref, Gen::Keep, Model::Network, glb16_shape,
     "fleet_glb16 form needs 6 -> hidden widths 1..256 -> 4 with at least one hidden layer", 64, "fleet_glb16 form needs K to be a multiple of 64", nullptr,
     nullptr, nullptr, false, prepare_fleet_glb16},
    {"glb44", true, Form::Glb44, Form::Glb44, kNoPref, Gen::Keep, Model::Network, glb44_shape, kGlb44Msg, kRolloutsPerWave,
     "glb44 form needs K to be a multiple of 16", nullptr, nullptr, nullptr, false, build_image},
    // the row form for every layer list of one to four hidden layers up to 32 wide (narrower layers padded with zeros): the reference's
    // order in every layer, up to three hidden layers / the output layer as a butterfly
    {"row32", false, Form::Row32, Form::Row32, kNoPref, Gen::Keep, Model::Network, row32_shape, kRow32Msg, kRolloutsPerWave,
     "row32 form needs K to be a multiple of 16", nullptr, nullptr, nullptr, false, build_image, 0, nullptr, row32_exact_depth, kRow32DepthMsg},
    {"row32_tree", false, Form::Row32Tree, Form::Row32Tree, kNoPref, Gen::Keep, Model::Network, row32_shape, kRow32TreeMsg, kRolloutsPerWave,
     "row32_tree form needs K to be a multiple of 16", nullptr, nullptr, nullptr, false, build_image},
    // the vector-ALU arm of the 64-wide A/B
    {"row64", false, Form::Row64R16, Form::Row64R16, kNoPref, Gen::Keep, Model::Any, form_shape, kRow64Msg},
    {"row64_r16", false, Form::Row64R16, Form::Row64R16, kNoPref, Gen::Keep, Model::Any, form_shape, kRow64Msg},
    {"oct", false, Form::Oct, Form::Oct, kNoPref, Gen::Off, Model::Any, form_shape, kOctMsg},
    {"oct_gen", false, Form::Oct, Form::Oct, kNoPref, Gen::On, Model::Any, form_shape, kOctMsg},
    {"multi2", false, Form::Multi2, Form::Multi2, kNoPref, Gen::Off, Model::Any, form_shape, kMultiMsg, 32, kMultiK},
    {"multi2_gen", false, Form::Multi2, Form::Multi2, kNoPref, Gen::On, Model::Any, form_shape, kMultiMsg, 32, kMultiK},
    {"multi4", false, Form::Multi4, Form::Multi4, kNoPref, Gen::Off, Model::Any, form_shape, kMultiMsg, 64, kMultiK},
    {"multi4_gen", false, Form::Multi4, Form::Multi4, kNoPref, Gen::On, Model::Any, form_shape, kMultiMsg, 64, kMultiK},
    // ND = 4, butterfly output layer
    {"multi4_tree", false, Form::Multi4Tree, Form::Multi4Tree, kNoPref, Gen::Off, Model::Any, form_shape, kMultiMsg, 64, kMultiK},
    {"multi4_tree_gen", false, Form::Multi4Tree, Form::Multi4Tree, kNoPref, Gen::On, Model::Any, form_shape, kMultiMsg, 64, kMultiK},
    {"fused", false, Form::Fused256, Form::Bf1, kNoPref, Gen::Keep},
    {"block256", false, Form::Fused256, Form::Bf1, kNoPref, Gen::Keep},
    {"block64", false, Form::Fused64, Form::Bf1, kNoPref, Gen::Keep},
};
}  // namespace

extern "C" {

const char *mppi_rollout_variant(const mppi_handle *h)
{
  if (!h) return "";
  static thread_local char buf[64];
  const FormDesc::Name &nm = form_desc(form_of(h)).name;
  const char *gen = (nm.gen && form_generator_noise(h)) ? "_gen" : "";
  switch (nm.tag) {
    case Tag::Fixed: return nm.stem;
    case Tag::HiddenLayers: snprintf(buf, sizeof(buf), "%s_h%d_l%d%s%s", nm.stem, h->hidden, h->n_hidden, nm.suffix, gen); break;
    case Tag::ForcedWaves:
      if (h->fleet_bf_waves == 0) return nm.stem;
      snprintf(buf, sizeof(buf), "%s_w%d", nm.stem, h->fleet_bf_waves);
      break;
    case Tag::LayersWidth: snprintf(buf, sizeof(buf), "%s_l%d_w%d", nm.stem, h->net.n_layers - 2, widest_hidden(h->net)); break;  // the forms of a layer list
  }
  return buf;
}

int mppi_set_rollout_variant(mppi_handle *h, const char *name)
{
  if (!h || !name) return MPPI_ERR_INVALID;
  DISARM(h);
  const Request *r = nullptr;
  int cap = -1;
  for (const Request &q : kRequests) {
    const size_t len = strlen(q.name);
    if (q.with_cap ? strncmp(name, q.name, len) != 0 : strcmp(name, q.name) != 0) continue;
    if (!q.with_cap || (cap = resident_cap_of(name + len)) >= -1) r = &q;
    break;
  }
  if (!r) return fail(h, MPPI_ERR_INVALID, "unknown variant");
  char msg[160];
  auto refuse = [&](const char *what) { return fail(h, MPPI_ERR_UNSUPPORTED, what); };
  if (r->model != Model::Any && h->basis != (r->model == Model::Basis)) {
    snprintf(msg, sizeof(msg), "%s is a form of the %s model", r->say ? r->say : r->name, r->model == Model::Basis ? "basis-function" : "network");
    return refuse(msg);
  }
  const Form f = h->basis ? r->bf : r->net;
  if (r->shape && !r->shape(h, f)) return refuse(r->shape_msg);
  if (r->shape2 && !r->shape2(h, f)) return refuse(r->shape2_msg);
  if (r->k_msg && h->K % r->k_multiple != 0) return refuse(r->k_msg);
  if (r->lds_bytes && r->lds_bytes(h->net) > r->lds_limit()) {
    snprintf(msg, sizeof(msg), "%s form: the weights of this layer list need %zu bytes of LDS per %s, %zu are available", r->name,
             r->lds_bytes(h->net), r->lds_unit, r->lds_limit());
    return refuse(msg);
  }
  if (r->needs_image && !image(h, form_desc(f).image)) {
    snprintf(msg, sizeof(msg), "%s form: this handle has no image", r->name);
    return refuse(msg);
  }
  if (r->prepare)
    if (int rc = r->prepare(h, f)) return rc;
  if (r->pref >= 0) h->pref = (Pref)r->pref;
  if (form_desc(f).cap) h->*form_desc(f).cap = cap;
  h->forced = f;
  h->fleet_bf_waves = r->waves;
  if (r->gen != Gen::Keep) h->multi_standalone_noise = r->gen == Gen::On;
  return MPPI_OK;
}

/* Test / tooling hook (not part of the drop-in surface): the rows of the selection table that match this handle's model, as
 * variant names a caller can pass to mppi_set_rollout_variant, best-first; returns how many were written (<= max_n). */
int mppi_debug_form_candidates(const mppi_handle *h, const char **names, int max_n)
{
  if (!h || !names || max_n <= 0) return 0;
  int n = 0;
  auto put = [&](const char *s) { for (int i = 0; i < n; i++) if (strcmp(names[i], s) == 0) return; if (n < max_n) names[n++] = s; };
  if (h->basis) { put("bf3"); put("quad"); put("fused"); return n; }
  if (!h->mfma_ok) { put("valu_lds"); return n; }
  for (const FormRule &r : kFormRules) {
    if ((r.hidden != 0 && r.hidden != h->hidden) || (r.n_hidden != 0 && r.n_hidden != h->n_hidden)) continue;
    if (!form_supported(r.form, h->hidden, h->n_hidden)) continue;
    const FormDesc::Ask &ask = form_desc(r.form).ask;
    if (h->K % ask.k_multiple != 0) continue;
    if (ask.first) put(ask.first);
    if (ask.second) put(ask.second);
  }
  return n;
}

}  // extern "C"
