// abi_internal.hpp -- what the files behind include/mppi_hip.h share: the handle, the kernel-form codes and the internal
// functions of one another.  mppi_abi.hip: handle life cycle, setters, getters; abi_forms.hip: which kernel form runs
// (selection table, names); abi_pack.hip: weight images and generator tables; abi_solve.hip: the solve pipeline (noise,
// rollout + tail launches, result polling, batched solves); abi_host.hip: the host-side halves of a tick (nominal replays,
// DDP feedback gains, the helper thread, the batched DDP pass and the batched nominal replay of a fleet on the device); abi_trace.hip: chosen rollouts of the last
// solve replayed with their records, for one handle or a whole fleet.
#pragma once
// mppi_abi.hip -- host side of libmppi_hip.so: the C ABI of include/mppi_hip.h.
//
// Owns one HIP stream and all device memory of a solver instance, enqueues one MPPI solve
// (PI/mppi_controller.cu:600-671) as: [H2D U|hist] -> noise -> rollout -> weights -> weighted
// reduction -> Savitzky-Golay -> [D2H scal|U], with ONE stream synchronisation per solve (the
// reference has three plus five blocking parameter uploads).
// There is no CPU fallback anywhere in this file: without a gfx950 device every compute entry
// point returns an error.
#include "../../include/mppi_hip.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <string>
#include <vector>

#include "mppi_kernels.hpp"
#include "ddp_feedback.hpp"
#include "basis_funcs.hpp"
#include "host_net.hpp"

namespace mppi_abi {

// Kernel forms of the rollout (abi_forms.hip has the table that picks one, and what each is).
enum class Form : int {
  Auto = 0,
  Fused64, Fused256,                // rollout_mfma.hip: one wave per 16 rollouts does everything (workgroups of 1 / 4 waves)
  Quad,                             // rollout_mfma.hip: network split over two waves + cost + control wave per 16 rollouts
  Oct,                              // rollout_oct.hip: 64-wide nets, four dynamics waves (one M tile each) + four riders
  Multi2, Multi4,                   // rollout_multi.hip: ND dynamics waves of 16 rollouts + riders
  Multi4Tree,                       // ... ND = 4 with the output layer as a butterfly over a rollout's four lanes
  Row, RowTree,                     // rollout_row.hip: 6-32-32-4 on the vector ALU; Tree: butterfly output layer
  Row64R16,                         // rollout_row64.hip: 64-wide nets on the vector ALU, 16 rollouts per group
  M44, M44Chain,                    // rollout_m44.hip: 64-wide nets on v_mfma_f32_4x4x1 with A-broadcast; hidden layers as two
                                    // accumulation chains (the automatic form) / Chain: one, the reference's order
  Lds44,                            // rollout_lds44.hip: any layer list up to 64 wide on v_mfma_f32_4x4x1, weights from LDS, every
                                    // layer one chain in the reference's order; by name only ("lds44")
  Lds128,                           // rollout_lds128.hip: any layer list up to 128 wide, a layer as two halves of 64 neurons with an
                                    // accumulator each, the reference's order; by name only ("lds128")
  Lds16,                            // rollout_lds16.hip: the throughput form of any layer list up to 128 wide: one wave per 16 rollouts on
                                    // v_mfma_f32_16x16x4, the A operands from an LDS image, the reference's order; by name only ("lds16")
  Glb16,                            // rollout_glb16.hip: lds16's wave for every layer list up to 256 wide: the head and the first R blocks of
                                    // the image resident in LDS, the other blocks read from global memory; by name only ("glb16", "glb16_r<N>")
  Glb44,                            // rollout_glb44.hip: lds128's group for every layer list up to 256 wide: a layer as one to four halves, the head
                                    // and the first R quads of the image resident in LDS, the other quads read from global memory; by name
                                    // only ("glb44", "glb44_r<N>")
  Fleet16,                          // rollout_fleet16.hip: lds16's wave and image with the argument block read from device memory: up to 64 handles
                                    // of one layer list share a launch (mppi_compute_control_batch); by name only ("fleet16")
  FleetMulti4,                      // rollout_fleet_multi.hip: Multi4Tree's workgroup with the stand-alone generator ("multi4_tree_gen"), the argument
                                    // block read from device memory: up to 64 handles of one standard shape share a launch; by name only
                                    // ("fleet_multi4"), no gated form
  FleetGlb16,                       // rollout_glb16.hip: glb16's wave and image with the argument block AND the layer list read from device memory: up to
                                    // 64 handles of ANY layer lists and caps share a launch; by name only ("fleet_glb16", "fleet_glb16_r<N>"), no
                                    // gated form
  ValuReg, ValuLds,                 // rollout_valu.hip: throughput-style vector kernels (any layer list: ValuLds)
  Bf1, Bf2, Bf3,                    // rollout_bf.hip: basis-function model, waves per 64 rollouts
  BfRow,                            // rollout_bf_row.hip: basis-function model in the row form's group (four dynamics waves + four
                                    // riders per 16 rollouts), the bits of Bf1..3; by name only ("bf_row")
  Row32, Row32Tree,                 // rollout_row32.hip: the row form (row_group.hpp) for any list of one to four hidden layers up to 32 wide, a
                                    // narrower layer padded with zeros; Row32: the reference's order in every layer, at most three hidden
                                    // layers; Tree: butterfly output layer; by name only ("row32", "row32_tree")
  FleetBf,                          // rollout_fleet_bf.hip: the workgroups of Bf1..3 with the argument block read from device memory and eps from
                                    // the stand-alone generator: up to 64 handles of the basis-function model share a launch; by name only
                                    // ("fleet_bf", "fleet_bf_w1..3"), no gated form
  Count
};
enum class Pref : int { Auto = 0, Mfma, Valu, ValuLds };

// Device images of the model's weights (abi_pack.hip: kImages says which handles have one, its size and how it is packed)
enum class Image : int {
  Theta = 0,  // the parameters as they were set (basis-function model: W[4][25])
  ThetaS,     // theta with hidden-layer biases * kTanhScale (register VALU kernel)
  Mfma,       // 6-HxN-4: register image of rollout_mfma.hip / rollout_multi.hip / rollout_oct.hip
  Row,        // 6-32-32-4: the weights in the register order of the row form (rollout_row.hip)
  BfRow,      // basis-function model: the per-lane image of rollout_bf_row.hip
  Row64,      // 64-wide nets: register + LDS image of rollout_row64.hip
  M44,        // 64-wide nets: image of rollout_m44.hip
  Lds44,      // any layer list with hidden widths <= 64: image of rollout_lds44.hip
  Lds128,     // any layer list with hidden widths <= 128 whose image fits the LDS: image of rollout_lds128.hip
  Lds16,      // the same lists: image of rollout_lds16.hip (and of rollout_fleet16.hip)
  Glb16,      // image of rollout_glb16.hip: only a handle that asked for "glb16" has one (built at that call)
  Glb44,      // image of rollout_glb44.hip: only a handle that asked for "glb44" has one (built at that call)
  Row32,      // one to four hidden layers up to 32 wide: the row form's register image for the list (rollout_row32.hip); only a handle
              // that asked for "row32" / "row32_tree" has one (built at that call)
  Trace,      // network model: k-major image of rollout_trace.hip (every layer's W transposed)
  Count
};
struct DeviceImage {
  float *d = nullptr;
  size_t bytes = 0;
};

struct Events {
  // e[0..3]: markers on the handle's stream before noise / before rollout / after rollout / after tail;
  // e[4], e[5]: begin and end of the rollout kernel's own dispatch (hipExtLaunchKernelGGL, MPPI_LAUNCH_ROLLOUT)
  hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

// Argument blocks that kernels read from DEVICE memory (the fleet forms): one device block, filled through a ring of pinned
// staging slots with one asynchronous copy per use.  All uses of a block go to ONE stream, which orders the copy into the device
// block behind the kernels that read its previous contents; a staging slot is written again only once the copy out of it has
// completed (its event).
struct ArgBlock {
  static constexpr int kRing = 4;
  unsigned char *d = nullptr, *h = nullptr;
  size_t slot = 0;  // bytes of the device block and of each staging slot
  hipEvent_t ev[kRing] = {nullptr, nullptr, nullptr, nullptr};
  bool used[kRing] = {false, false, false, false};
  int cur = 0;
};
hipError_t arg_block_create(ArgBlock &b, size_t slot_bytes);
void arg_block_destroy(ArgBlock &b);
hipError_t arg_block_stage(ArgBlock &b, unsigned char **host);            // the next staging slot, free to write
hipError_t arg_block_send(ArgBlock &b, size_t bytes, hipStream_t stream);  // its first `bytes` to the device block
}  // namespace mppi_abi
using mppi_abi::Events;


struct mppi_handle {
  using NetDesc = mppi::NetDesc;
  using DdpResult = mppi::DdpResult;
  using HostNetFma = mppi::HostNetFma;
  mppi_config cfg{};
  int K = 0, T = 0, k99 = 0;
  float dt = 0.0f;
  NetDesc net{};
  bool mfma_ok = false;
  int hidden = 0, n_hidden = 0;
  mppi_abi::Pref pref = mppi_abi::Pref::Auto;   // "auto" | "mfma" | "valu" | "valu_lds"
  mppi_abi::Form forced = mppi_abi::Form::Auto;  // a kernel form asked for by name (mppi_set_rollout_variant); Auto: the selection table
  bool multi_standalone_noise = false;  // multi form: eps from the stand-alone generator kernel instead of the control wave
  int num_simds = 1024;     // 4 per CU
  hipStream_t stream = nullptr;
  // The stream the handle's most recent device work went to: its own, or the device's batch stream after a
  // batched solve (mppi_compute_control_batch).  nullptr: nothing outstanding anywhere but on `stream`.
  hipStream_t order_stream = nullptr;
  int n_slots = 1;  // explicit-noise slots in d_noise: one per iteration
  bool u_dirty = true;          // host copy of U/hist differs from the device copy in d_in
  unsigned seq = 0;             // sequence number of the last enqueued solve (last word of every h_res entry)
  std::vector<float> sg_buf;    // scratch of the host-side Savitzky-Golay pass
  bool basis = false;  // GeneralizedLinear basis-function dynamics (cfg.n_layers == 0); theta holds W[4][25]
  // DDP feedback gains (row f2): weights of initDDP (mppi_controller.cu:410-417) and the last result
  float ddp_Q[7] = {0.5f, 0.5f, 0.25f, 0.0f, 0.05f, 0.01f, 0.01f};
  float ddp_R[2] = {10.0f, 10.0f};
  float ddp_Qf[7] = {0, 0, 0, 0, 0, 0, 0};
  DdpResult ddp;
  bool have_ddp = false;
  int ddp_on_device = 0;  // the last DDP pass ran in ddp_fleet_kernel (mppi_compute_feedback_gains_batch), not on the host
  int nominal_on_device = 0;  // the last nominal replay ran in nominal_fleet_kernel (mppi_nominal_traj_batch), not on the host
  int nominal_gains_fused = 0;  // the last mppi_nominal_and_gains_batch ran in nominal_gains_fleet_kernel, not as the two calls
  int closed_loop_on_device = 0, closed_loop_ticks = 0;  // the last mppi_closed_loop_ticks_batch: its ticks were enqueued on the device's batch stream with
                                                         // the plant step in plant_fleet_kernel (not the loop of public calls); the ticks it completed
  // mppi_set_plant_model: the network of the plant that mppi_plant_drive_batch and mppi_closed_loop_sim_batch step -- its layer
  // list, its parameters, its host twin and its trace image (pack_trace_weights) in d_plant_img, which is allocated once for the
  // largest image a layer list can have and freed with the handle (so that a change never frees device memory beside an armed
  // solve).  have_plant == false: the plant is the handle's own network with the handle's negate_yaw_der.
  bool have_plant = false;
  NetDesc plant_net{};
  int plant_negate = 0;
  std::vector<float> plant_theta;
  HostNetFma plant_hnet;
  float *d_plant_img = nullptr;
  int plant_drive_on_device = 0;  // the last mppi_plant_drive_batch ran in plant_drive_fleet_kernel, not in the host text
  int trace_on_device = 0;  // the last trace ran in the fleet's kernels (mppi_trace_rollouts_batch), not in a launch of the handle's own
  hipStream_t batch_s = nullptr;  // the device's batch stream, looked up once (mppi_compute_control_batch)
  unsigned *d_counter = nullptr;  // [1 + T] arrival counters of the tail kernel
  float *d_part = nullptr;        // [T][K/64][2] chain results of the tail kernel when K > 4096
  // K > 4096 (one-launch streaming tail): d_part holds 8-byte {value, epoch} granules; d_gx the granules of
  // the column exchanges; tail_epoch the tag of the last tail launch; tail_poll_ticks the deadline of its waits (100 MHz ticks)
  unsigned long long *d_gx = nullptr;
  // the rollout launch's minimum cost on its way to the tail kernel (mppi_device.hpp: publish_min_cost): kMinCostLines keys, all
  // ones when allocated; the tag of the latest rollout launch that wrote d_costs (next_min_cost_tag); MPPI_MIN_COST=0: not used
  unsigned long long *d_min_cost = nullptr;
  unsigned min_cost_tag = 0;
  bool use_min_cost = true;
  unsigned long long *d_ug = nullptr;  // [T][2] granules of the raw weighted mean: row workgroups -> the smoothing workgroup
  unsigned tail_epoch = 0, tail_poll_ticks = 2000000;  // 20 ms
  float *d_res_map = nullptr;   // device-side address of the host-mapped result block h_res

  std::vector<float> U, hist, theta, map_rgba;
  HostNetFma hnet;  // host twin of the network for computeNominalTraj (rebuilt with every mppi_set_nn_params)
  int map_w = 0, map_h = 0;
  mppi_cost_params cost{};
  float r_c1[3] = {0, 0, 0}, r_c2[3] = {0, 0, 0}, trs[3] = {0, 0, 1};
  float u_lo[2] = {0, 0}, u_hi[2] = {0, 0};
  bool have_nn = false, have_map = false, have_cost = false;

  float *d_in = nullptr, *d_scal = nullptr;
  float *d_in_buf[2] = {nullptr, nullptr};  // d_in points at one of them; the tail kernel leaves the
  int in_cur = 0;                            // stride-slid copy of [U | hist] in the other one
  bool slid_valid = false;
  float *d_noise = nullptr, *d_stage = nullptr;
  // Generator-kernel forms: eps of a solve is drawn by the stand-alone kernel into one of two buffers, on a
  // stream of its own (all generator launches, in order: the MRG32k3a states advance in launch order); the
  // draws of the NEXT solve are requested as soon as this solve's rollout has been enqueued and start when
  // that rollout ends, i.e. they overlap the weights / tail kernels, which leave the chip idle.
  float *d_gen[2] = {nullptr, nullptr};
  int gen_cur = 0;             // buffer of the most recent generator-mode solve (holds its applied controls V)
  bool gen_async = false;      // K T >= 2^20: generator on its own stream, next solve's draws prefetched
  bool prefetch_valid = false; // d_gen[1 - gen_cur] holds the next solve's draws (ev_gen marks their completion)
  float *v_buf = nullptr;      // where the last solve's applied controls are
  hipStream_t gstream = nullptr;
  hipEvent_t ev_gen = nullptr, ev_s1 = nullptr;
  // stage timing of the asynchronous generator: begin / end of the generator launch on gstream that was enqueued
  // during a timed solve (it runs BESIDE that solve's rollout or tail: reported as noise_ms, not additive)
  hipEvent_t ev_gt[2] = {nullptr, nullptr};
  bool gen_timed = false, gen_time_now = false;
  float *d_costs = nullptr, *d_w = nullptr;
  float *d_map = nullptr;
  mppi_abi::DeviceImage img[(int)mppi_abi::Image::Count];  // the weight images this handle has (d == nullptr: not this one)
  mppi_abi::ArgBlock *fleet_one = nullptr;  // "fleet16", "fleet_multi4", "fleet_bf", "fleet_glb16": the argument block of this handle's own launches (on its own stream); only a
                                 // handle that asked for the form has one
  int glb16_cap = -1;            // "glb16_r<N>", "fleet_glb16_r<N>": the cap on the resident stream blocks; -1: none
  int glb44_cap = -1;            // "glb44_r<N>": the cap on the resident stream quads; -1: none
  int fleet_bf_waves = 0;        // "fleet_bf_w<N>": the wave count of the fleet's launch forced; 0 ("fleet_bf"): fleet_bf_plan chooses
  // mppi_trace_rollouts: the records of one chunk of trace_chunk rollouts -- states [c][T][7], controls [c][T][2], step costs
  // [c][T], costs [c], first_crash [c] (int) -- allocated with the handle (nothing is allocated or freed while armed); the
  // chunk's rollout indices reach the kernel through host-mapped memory (h_trace_ks / d_trace_ks: no upload on the stream)
  float *d_trace = nullptr;
  int *h_trace_ks = nullptr, *d_trace_ks = nullptr;
  int trace_chunk = 0;
  float solve_state[7] = {0, 0, 0, 0, 0, 0, 0};  // the vehicle state of the most recent solve (what v_buf and d_costs belong to)
  bool have_solve = false;     // solve_state, v_buf and d_costs belong together (cleared where a solve starts to repoint v_buf)
  bool have_weights = false;   // ... and d_w too: a whole solve, not mppi_rollout_only
  bool valu_reg_ok = false;
  double *d_invt = nullptr;
  uint32_t *d_rng[2] = {nullptr, nullptr};
  uint32_t *d_jump = nullptr, *d_sub = nullptr, *d_one = nullptr;
  int rng_cur = 0;
  int noise_L = 1, noise_C = 1;
  float *h_in = nullptr, *h_res = nullptr;
  // >0: d_noise holds that many explicit iterations for the next solve.  Only ever 0 or cfg.num_iters: mppi_set_noise accepts
  // exactly num_iters iterations and is its one writer of a non-zero value, every solve resets it, and cfg.num_iters is fixed at
  // mppi_create (a batch shares one num_iters besides) -- so no solve checks that the count fits its iterations.
  int explicit_iters = 0;
  bool pending = false;       // a solve is enqueued, results not yet collected
  bool pending_timed = false;
  bool pending_armed = false;  // the pending solve is one that was armed (mppi_arm): wait_pending checks its rows too
  float traj_cost = 0.0f, baseline = 0.0f, eta = 0.0f;

  int spin_budget = 0, fault_wave = 0;  // mppi_debug_inject_handover_fault (0, 0: kSpinBudget, no fault)
  // mppi_debug_capture_iterations: [num_iters][2T + K] -- the raw weighted mean U and the costs after every iteration
  float *d_cap = nullptr;
  bool capture = false, cap_valid = false, cap_explicit = false;
  double wait_timeout_s = 30.0;  // mppi_set_wait_timeout
  // solve-ahead (mppi_arm, mppi_control_ticks, abi_solve.hip): the gate block of the solve enqueued one tick ahead --
  // kGateReplicas copies of [state[7], gate word], device memory the host stores into through the PCIe BAR where the
  // platform allows it (gate_bar), else host-mapped memory; gate_cpu is the pointer the host writes, d_gate what the kernel reads
  unsigned *gate_cpu = nullptr, *d_gate = nullptr;
  bool gate_bar = false;
  bool chain = true;   // mppi_debug_set_chained_ticks
  // The gate block is double-buffered (gate_blk: the block of the latest gated solve; gate_host / gate_dev below): the tail of a
  // gated solve still reads hist from its block after the host has seen its result, when the next gated solve's gate is written.
  int gate_blk = 0;
  // solve-ahead (mppi_arm, abi_solve.hip): the handle's NEXT solve is enqueued, gated, and waits for the next compute call
  int armed = 0;                 // 0: not armed; 1: a latency form with its in-kernel generator; 2: the multi4-tree form with the
                                 // prefetched generator kernel (abi_solve.hip: arm_kind)
  unsigned arm_seq = 0;          // the armed solve's sequence number (its gate word)
  unsigned seq_floor = 0;        // a called-off solve published under this number: every later solve takes a larger one
  int arm_in = 0;                // d_in_buf the armed solve's tail smooths into (its slid copy: the other one)
  float *arm_vbuf = nullptr;     // where the armed solve leaves its applied controls
  bool arm_publish_only = false;  // its tail only publishes (inside mppi_control_ticks): the device copy of [U | hist] is stale
  int arm_n = 0;                 // > 0: armed in one launch together with arm_peers[0 .. arm_n) (mppi_arm_batch)
  mppi_handle *arm_peers[4] = {nullptr, nullptr, nullptr, nullptr};
  hipStream_t arm_stream = nullptr;  // the stream the armed solve went to (the handle's own, or the device's batch stream)
  hipEvent_t ev_arm = nullptr;   // recorded on arm_stream in front of the armed solve: readers of the last result wait for it alone
  std::chrono::steady_clock::time_point arm_until;  // the host's deadline for opening the gate (a margin inside max_wait_s)
  // the armed solve writes its costs and weights into the second pair (swapped in when its gate opens): the last result's
  // vectors stay readable while it is armed, and a solve called off leaves them alone
  float *d_costs_alt = nullptr, *d_w_alt = nullptr;
  // mppi_debug_launch_info: how many instances the rollout launch of the most recently enqueued solve served (an armed solve
  // counts; 0: no solve yet) and whether it was a gated launch -- written where the launch is made
  int launch_instances = 0;
  bool launch_gated = false;
  bool timed_out = false;        // a wait ran out of time and that solve's device work may still run: recover_timed_out (abi_solve.hip)
  bool no_result = false;        // the last solve was lost (timeout): mppi_get_results refuses until a solve completes
  bool timing = false;
  int timing_every = 1;      // record stage events on every Nth solve only (events add launch gaps)
  unsigned timing_count = 0;
  std::vector<Events> ev;  // one set per iteration
  mppi_stage_times acc{};
  std::string err;
};

namespace mppi_abi {
using namespace mppi;


#define HIPCHK(h, call)                                                  \
  do {                                                                   \
    hipError_t e__ = (call);                                             \
    if (e__ != hipSuccess) return fail((h), MPPI_ERR_HIP, #call, e__);   \
  } while (0)
// The calling thread's current device is `dev` afterwards: hipGetDevice (a thread-local read, 0.07 us) and hipSetDevice only
// when it differs -- a control loop calls the solve entries from one thread whose device never changes.
inline hipError_t ensure_device(int dev)
{
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur == dev) return hipSuccess;
  return hipSetDevice(dev);
}
#define OWN(h)                      \
  do {                              \
    int rc__ = own_stream(h);       \
    if (rc__) return rc__;          \
  } while (0)

int compute_k99(int K);
// a table with one row per member of an enum (whose last member is Count): row i describes member i
template <class Row, class Id, size_t N>
constexpr bool rows_in_order(const Row (&rows)[N], Id Row::*id)
{
  for (size_t i = 0; i < N; i++)
    if ((size_t)(rows[i].*id) != i) return false;
  return N == (size_t)Id::Count;
}
// abi_pack.hip: one row per weight image, indexed by Image
struct ImageDesc {
  Image id;                                           // the row's own index
  bool (*has)(const mppi_handle *h);                  // which handles have it
  size_t (*floats)(const mppi_handle *h);             // its size
  std::vector<float> (*pack)(const mppi_handle *h);   // from h->theta
  bool on_request;          // built when mppi_set_rollout_variant asks for its form (upload_image allocates it), not with the handle
  const char *size_check;   // the refusal where the packed size is not the allocated one; nullptr: not checked
};
const ImageDesc &image_desc(Image id);  // row id of the table
inline float *image(const mppi_handle *h, Image id) { return h->img[(int)id].d; }
// abi_pack.hip: Image::Trace's packing for any network (mppi_set_plant_model packs the plant's with it)
std::vector<float> pack_trace_weights(const std::vector<float> &theta, const mppi::NetDesc &net);
int upload_image(mppi_handle *h, Image id);  // packs the image from h->theta and copies it (an image built on request: allocated at the first call)
int upload_images(mppi_handle *h);           // every image the handle has, and the one the form it asked for by name needs
int seed_device(mppi_handle *h, uint64_t seed, uint64_t offset);
int upload_rng_tables(mppi_handle *h);
bool use_mfma(const mppi_handle *h);
bool use_valu_reg(const mppi_handle *h);
Form form_of(const mppi_handle *h);
bool form_generator_noise(const mppi_handle *h);
bool has_noise_wave(const mppi_handle *h);

// abi_forms.hip: what the host knows about a rollout form, one row per form, indexed by Form
struct FormDesc;
using LaunchFn = hipError_t (*)(mppi_handle *h, const FormDesc &d, const RolloutArgs &a, hipStream_t stream);
using BatchFn = hipError_t (*)(const mppi_handle *h0, const FormDesc &d, const QuadBatchArgs &qb, hipStream_t stream);
// hs: the n handles of the launch (a form of one list and one shape reads hs[0]); d_nets: the instances' layer lists in device memory (fleet_net)
using FleetFn = hipError_t (*)(mppi_handle *const *hs, const RolloutArgs *h_inst, const RolloutArgs *d_inst, const FleetGlbNet *d_nets, int n, hipStream_t stream);
enum class Noise { Never, InKernel, UnlessStandalone };  // does the kernel draw eps itself?  UnlessStandalone (oct, multi): unless the
                                                          // stand-alone generator was asked for ("_gen") or is the automatic choice
enum class Tag { Fixed, HiddenLayers, LayersWidth, ForcedWaves };  // the reported name: stem [+ "_h%d_l%d" | "_l%d_w%d"] + suffix [+ "_gen"];
                                                                   // ForcedWaves: stem [+ "_w%d" where the handle forces a wave count]
enum : unsigned {
  kGate = 1,       // has a gated kernel (mppi_arm): the latency forms with riders
  kPublishes = 2,  // publishes its minimum cost for the streaming tail (multi_group.hpp)
  kByName = 4,     // runs by name only, for every model it serves
  kNegateYaw = 8,  // forces negate_yaw_der (bf_row: its kinematics are the riders'; computeKinematics of the basis-function model
                   // always negates the yaw rate, generalized_linear.cu:212-217 -- the model's own kernels never look at the flag)
};
struct FormDesc {
  Form form;       // the row's own index
  Image image;     // RolloutArgs::wpack
  Noise noise;
  unsigned flags;  // kGate | ...
  bool (*shape)(int hidden, int n_hidden);  // the standard shapes 6 -> hidden x n_hidden -> 4 it exists for; nullptr: not a form of those
  LaunchFn launch;
  int arg;         // what the launch adapter passes on: waves (bf), ND code (multi), block threads (mfma), rollouts per group (row64), tree / split
  struct Batch {   // one launch for the handles of a batch (batch_together); launch == nullptr: none
    BatchFn launch = nullptr;
    bool pair_only = false;   // the pair of a tick only; else up to kMaxBatch
    bool same_list = false;   // the whole layer list must agree, not only hidden x n_hidden
    int waves = 0;            // waves per 64 rollouts that need a SIMD of their own
  } batch;                    // (a form with a resident cap batches only handles of one cap)
  FleetFn fleet;              // the launch shared by a fleet (mppi_compute_control_batch); != nullptr: a fleet form
  int mppi_handle::*cap;      // "<form>_r<N>": where the handle keeps the cap on the resident part; nullptr: the form has none
  struct Name {
    const char *stem;
    Tag tag = Tag::Fixed;
    const char *suffix = "";
    bool gen = false;         // takes "_gen" where eps comes from the stand-alone generator
  } name;
  struct Ask {                // mppi_debug_form_candidates: the requests that time this form where kFormRules names it
    const char *first = nullptr, *second = nullptr;
    int k_multiple = 1;
  } ask;
  // a fleet form whose instances bring their own layer lists: the handle's entry of the fourth section of the fleet's argument block
  // (behind the generator descriptors); nullptr: the form has no such section
  FleetGlbNet (*fleet_net)(const mppi_handle *h) = nullptr;
  bool has(unsigned f) const { return (flags & f) != 0; }
};
const FormDesc &form_desc(Form f);  // row f of the table
hipStream_t batch_stream(int device);
// abi_solve.hip: the argument block beside a device's batch stream, shared by every fleet on the device and never destroyed.
// mu: held while a batched solve, a batched DDP pass or a batched nominal replay stages, sends and launches (the latter two: until
// their results are back)
struct FleetBlock {
  std::mutex mu;
  ArgBlock args;
  bool ready = false;
};
FleetBlock *fleet_block(int device);
void fill_cost_args(const mppi_handle *h, CostArgs &c);
void fill_rollout_args(const mppi_handle *h, const float *state, float *noise, RolloutArgs &a);
// a rollout launch that is followed by its tail kernel: the tag its minimum cost travels under (a.min_cost, a.min_cost_tag)
int tag_min_cost(mppi_handle *h, RolloutArgs &a, hipStream_t stream);
int launch_rollout(mppi_handle *h, const RolloutArgs &a);
hipError_t launch_rollout_fleet_one(mppi_handle *h, const RolloutArgs &a);  // a handle of a fleet form solved alone
// what a handle that asks for a fleet form needs of its own (fleet_one: its argument block and, with_net, one layer-list descriptor behind it)
int fleet_prepare(mppi_handle *h, bool with_net);
int check_ready(mppi_handle *h);
int launch_generator(mppi_handle *h, float *dst);
int acquire_noise(mppi_handle *h, float **buf_out);
int prefetch_noise(mppi_handle *h);
int upload_controls_if_dirty(mppi_handle *h, hipStream_t stream);
void savgol_host(mppi_handle *h, const float *src, int stride, int off1);
bool wants_slid_copy(const mppi_handle *h);
TailLaunch tail_launch(const mppi_handle *h, const float *V, bool last);
int fail(mppi_handle *h, int code, const char *what, hipError_t e = hipSuccess);
int recover_timed_out(mppi_handle *h);
bool gen_beside_rollout(const mppi_handle *h);
int own_stream(mppi_handle *h);
void free_all(mppi_handle *h);

// the gate block of the latest gated solve: the host's pointer and the kernels'; blocks lie gate_block_stride floats apart
inline size_t gate_block_stride(int T) { return (gate_block_floats(T) + 63) & ~(size_t)63; }
inline unsigned *gate_host(const mppi_handle *h) { return h->gate_cpu + (size_t)h->gate_blk * gate_block_stride(h->T); }
inline const unsigned *gate_dev(const mppi_handle *h) { return h->d_gate + (size_t)h->gate_blk * gate_block_stride(h->T); }
// abi_solve.hip: the armed solve is called off (its gate opened with the cancel bit; never blocks on the device); the handle's
// generator stream is put back where it was.  Every call that changes what the armed solve would compute calls this first.
int solve_ahead_disarm(mppi_handle *h);
#define DISARM(h)                           \
  do {                                      \
    int rc__ = solve_ahead_disarm(h);       \
    if (rc__) return rc__;                  \
  } while (0)

// where small follow-up work (upload of U, the slide kernel) goes: behind the handle's latest work, wherever it is
inline hipStream_t work_stream(const mppi_handle *h) { return h->order_stream ? h->order_stream : h->stream; }

// the vehicle state a solve (or mppi_rollout_only) runs from, kept for mppi_trace_rollouts
// forget_solve_state where a solve starts to repoint v_buf, note_solve_state once it is enqueued: a solve whose launch failed
// leaves nothing to trace instead of an old state beside a new buffer.
inline void forget_solve_state(mppi_handle *h) { h->have_solve = h->have_weights = false; }
inline void note_solve_state(mppi_handle *h, const float *state, bool with_weights)
{
  memcpy(h->solve_state, state, sizeof(h->solve_state));
  h->have_solve = true;
  h->have_weights = with_weights;
}
constexpr int kTraceChunk = 1024;  // rollouts per launch of mppi_trace_rollouts

// abi_host.hip: the helper thread of the paired host work (mppi_set_host_threads)
extern std::atomic<int> g_host_threads;
void host_helper_arm();
// abi_host.hip: the sharing rule of the batched nominal replay (mppi_nominal_traj_batch; the closed loop of a fleet asks it too)
bool nominal_fleet_together(mppi_handle *const *hs, int n);
// abi_host.hip: the plant of a handle (mppi_set_plant_model; else the handle's own network) and what of a PlantDriveArgs block is the
// same for the batched call and the closed loop: the plant's image and layer list, negate_yaw_der, dt / substeps, the handle's
// limits, the interpolation weights, where the image goes.  The pointers are the caller's.
const NetDesc &plant_net_of(const mppi_handle *h);
void plant_drive_fill(const mppi_handle *h, int periods, int substeps, int feedback, PlantDriveArgs &a);
// the sharing rule of mppi_plant_drive_batch (the closed loop of a fleet asks it too)
bool plant_drive_together(mppi_handle *const *hs, int n);
// abi_solve.hip: the host's check behind a closed-loop run on the device (mppi_closed_loop_ticks_batch) over one handle's logs -- etas
// [n_ticks], controls [n_ticks][stride][2]: the first tick whose eta is below 1 or not finite or whose applied controls are not
// finite; -1: none
int closed_loop_first_bad_tick(const float *etas, const float *controls, int n_ticks, int stride);

// The buffers of a batched host pass: ONE set per purpose and device beside the device's batch stream, grown on demand and never
// destroyed -- the instances' inputs (pinned staging -> device, one copy), their results (device -> pinned, one copy) and, where
// the kernel keeps records, its work area.  Used under the device's FleetBlock::mu, from staging until the results are unpacked;
// the stream is idle in them whenever the mutex is free.
struct FleetWork {
  float *d_in = nullptr, *d_out = nullptr, *d_work = nullptr, *h_in = nullptr, *h_out = nullptr;
  size_t in_cap = 0, out_cap = 0, work_cap = 0;  // floats
};

inline hipError_t fleet_grow(float **d, float **h, size_t *cap, size_t need)
{
  if (need <= *cap) return hipSuccess;
  const size_t want = need + need / 2;
  if (*d) (void)hipFree(*d);
  if (h && *h) (void)hipHostFree(*h);
  *d = nullptr;
  if (h) *h = nullptr;
  *cap = 0;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(d), sizeof(float) * want);
  if (e == hipSuccess && h) e = hipHostMalloc(reinterpret_cast<void **>(h), sizeof(float) * want, hipHostMallocDefault);
  if (e != hipSuccess) {
    if (*d) (void)hipFree(*d);
    *d = nullptr;
    return e;
  }
  *cap = want;
  return hipSuccess;
}

inline size_t align4(size_t floats) { return (floats + 3) & ~(size_t)3; }

// One batched host pass over the handles hs[0 .. n) of one device (abi_host.hip: the DDP passes and the nominal replays of a fleet;
// abi_trace.hip: its traces): open() -- the device, its batch stream and fleet block, every handle's offsets into the buffers, the
// block's lock (held until the pass goes out of scope), the buffers, the inputs staged by the caller and sent in one copy;
// launch() -- the argument blocks of one chunk of at most kMaxFleet handles staged, sent and its kernel enqueued (a chunk's blocks
// are ordered behind the launch before it, which reads the device block); finish() -- the results in one copy and the
// synchronise.  An error of the enqueues is kept in `e`: the calls after it do nothing and finish() fails every handle with
// `what`.  The results are in w->h_out, at out_off, once finish() has returned MPPI_OK.
struct FleetPass {
  mppi_handle *const *hs;
  int n;
  const char *what;
  hipStream_t S = nullptr;
  FleetBlock *fb = nullptr;
  FleetWork *w = nullptr;
  std::vector<size_t> in_off, out_off, work_off;  // [n + 1] floats, every handle's piece a multiple of four
  std::unique_lock<std::mutex> lk;
  hipError_t e = hipSuccess;

  // in_floats(i) / out_floats(i) / work_floats(i): handle i's pieces (0: none); stage(i, in): fills handle i's inputs in pinned memory
  template <class InFloats, class OutFloats, class WorkFloats, class Stage>
  int open(FleetWork *work, InFloats in_floats, OutFloats out_floats, WorkFloats work_floats, Stage stage)
  {
    mppi_handle *h0 = hs[0];
    const int dev = h0->cfg.device;
    HIPCHK(h0, ensure_device(dev));
    S = batch_stream(dev);
    if (!S) return fail(h0, MPPI_ERR_HIP, "no batch stream");
    fb = fleet_block(dev);
    if (!fb) return fail(h0, MPPI_ERR_HIP, "no argument block for the fleet");
    in_off = out_off = work_off = std::vector<size_t>((size_t)n + 1, 0);
    for (int i = 0; i < n; i++) {
      in_off[i + 1] = in_off[i] + align4(in_floats(i));
      out_off[i + 1] = out_off[i] + align4(out_floats(i));
      work_off[i + 1] = work_off[i] + align4(work_floats(i));
    }
    lk = std::unique_lock<std::mutex>(fb->mu);
    w = &work[dev];
    if (in_off[n] > w->in_cap || out_off[n] > w->out_cap || work_off[n] > w->work_cap) {
      HIPCHK(h0, hipStreamSynchronize(S));  // nothing of an earlier pass is behind the buffers; nothing else on the stream reads them
      HIPCHK(h0, fleet_grow(&w->d_in, &w->h_in, &w->in_cap, in_off[n]));
      HIPCHK(h0, fleet_grow(&w->d_out, &w->h_out, &w->out_cap, out_off[n]));
      HIPCHK(h0, fleet_grow(&w->d_work, nullptr, &w->work_cap, work_off[n]));
    }
    for (int i = 0; i < n; i++) stage(i, w->h_in + in_off[i]);
    if (in_off[n] > 0) e = hipMemcpyAsync(w->d_in, w->h_in, sizeof(float) * in_off[n], hipMemcpyHostToDevice, S);
    return MPPI_OK;
  }

  // handles [at, at + m): fill(i, a) writes handle i's (zeroed) argument block
  template <class Args, class Fill>
  void launch(int at, int m, hipError_t (*kernel)(const Args *, const Args *, int, hipStream_t), Fill fill)
  {
    unsigned char *host = nullptr;
    if (e != hipSuccess || (e = arg_block_stage(fb->args, &host)) != hipSuccess) return;
    Args *args = reinterpret_cast<Args *>(host);
    for (int i = at; i < at + m; i++) {
      args[i - at] = Args{};
      fill(i, args[i - at]);
    }
    e = arg_block_send(fb->args, sizeof(Args) * (size_t)m, S);
    if (e == hipSuccess) e = kernel(args, reinterpret_cast<const Args *>(fb->args.d), m, S);
  }

  int finish()
  {
    if (e == hipSuccess && out_off[n] > 0) e = hipMemcpyAsync(w->h_out, w->d_out, sizeof(float) * out_off[n], hipMemcpyDeviceToHost, S);
    if (e == hipSuccess) e = hipStreamSynchronize(S);
    if (e == hipSuccess) return MPPI_OK;
    (void)hipStreamSynchronize(S);  // nothing enqueued so far is left behind the buffers
    for (int i = 0; i < n; i++) fail(hs[i], MPPI_ERR_HIP, what, e);
    return MPPI_ERR_HIP;
  }
};

}  // namespace mppi_abi
