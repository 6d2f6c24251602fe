// abi_solve.hip -- one MPPI solve (PI/mppi_controller.cu:600-671) as launches on a stream: noise source, rollout kernel, tail
// kernel, polling of the host-mapped result block; result getters.  "Enqueue a solve for n >= 1 handles" is written once, as
// phases (collect, begin_solves, distrust, solve_step, finish_solves: "the phases of a solve" below); three short drivers say
// how the argument blocks the phases fill reach the device -- enqueue_solve (one handle, its own stream), enqueue_pair (2-4
// handles, one rollout launch), enqueue_fleet (2-64 handles of a fleet form, three launches).  closed_loop_fleet is enqueue_fleet's
// tick n_ticks times over with the plant step between two ticks and nothing collected (mppi_closed_loop_ticks_batch; with a plant of
// its own under the drive law: mppi_closed_loop_sim_batch).
#include "abi_internal.hpp"

using namespace mppi;
using namespace mppi_abi;

namespace mppi_abi {

// Batched solves of several handles go to ONE stream per device, shared by all handles and never destroyed, so
// that the instances' kernels are one launch and a handle never holds another handle's stream.
std::mutex g_batch_mu;
hipStream_t g_batch_stream[64] = {};
hipStream_t batch_stream(int device)
{
  if (device < 0 || device >= 64) return nullptr;
  std::lock_guard<std::mutex> lk(g_batch_mu);
  if (!g_batch_stream[device] &&
      hipStreamCreateWithFlags(&g_batch_stream[device], hipStreamNonBlocking) != hipSuccess)
    g_batch_stream[device] = nullptr;
  return g_batch_stream[device];
}

hipError_t arg_block_create(ArgBlock &b, size_t slot_bytes)
{
  b.slot = (slot_bytes + 255) & ~(size_t)255;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&b.d), b.slot);
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&b.h), b.slot * ArgBlock::kRing, hipHostMallocDefault);
  for (int i = 0; i < ArgBlock::kRing && e == hipSuccess; i++) e = hipEventCreateWithFlags(&b.ev[i], hipEventDisableTiming);
  if (e != hipSuccess) arg_block_destroy(b);
  return e;
}

void arg_block_destroy(ArgBlock &b)
{
  for (hipEvent_t &e : b.ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  if (b.h) (void)hipHostFree(b.h);
  if (b.d) (void)hipFree(b.d);
  b.h = b.d = nullptr;
}

hipError_t arg_block_stage(ArgBlock &b, unsigned char **host)
{
  if (b.used[b.cur]) {  // the copy out of this slot, kRing uses ago: long complete as a rule
    if (hipError_t e = hipEventSynchronize(b.ev[b.cur]); e != hipSuccess) return e;
    b.used[b.cur] = false;
  }
  *host = b.h + b.slot * (size_t)b.cur;
  return hipSuccess;
}

hipError_t arg_block_send(ArgBlock &b, size_t bytes, hipStream_t stream)
{
  if (bytes > b.slot) return hipErrorInvalidValue;
  hipError_t e = hipMemcpyAsync(b.d, b.h + b.slot * (size_t)b.cur, bytes, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipEventRecord(b.ev[b.cur], stream);
  if (e != hipSuccess) return e;
  b.used[b.cur] = true;
  b.cur = (b.cur + 1) % ArgBlock::kRing;
  return hipSuccess;
}

// The argument blocks of a fleet form's batched solve ("fleet16", "fleet_multi4", "fleet_bf", "fleet_glb16"): ONE block per device beside the device's batch stream, shared by every
// fleet on the device and never destroyed -- per iteration the rollout, tail and generator blocks of up to kMaxFleet instances,
// packed for the fleet's n, and behind them -- for a form whose instances bring their own layer lists (FormDesc::fleet_net) -- the
// instances' list descriptors (FleetBlock: abi_internal.hpp).  A batched DDP pass and a batched nominal replay (abi_host.hip) send their
// instances' blocks through it too.
static FleetBlock g_fleet[64];
static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
static size_t fleet_tail_offset(int n) { return align16(sizeof(RolloutArgs) * (size_t)n); }
static size_t fleet_noise_offset(int n) { return align16(fleet_tail_offset(n) + solve_tail_fleet_arg_bytes() * (size_t)n); }
static size_t fleet_net_offset(int n) { return align16(fleet_noise_offset(n) + sizeof(NoiseFleetDesc) * (size_t)n); }
static size_t fleet_bytes(int n, bool with_nets) { return with_nets ? align16(fleet_net_offset(n) + sizeof(FleetGlbNet) * (size_t)n) : fleet_net_offset(n); }
FleetBlock *fleet_block(int device)
{
  if (device < 0 || device >= 64) return nullptr;
  std::lock_guard<std::mutex> lk(g_batch_mu);
  FleetBlock &fb = g_fleet[device];
  // (the largest of the uses: a batched solve's blocks, a batched DDP pass's, a batched nominal replay's, a batched trace's)
  if (!fb.ready)
    fb.ready = arg_block_create(fb.args, std::max({fleet_bytes(kMaxFleet, true), sizeof(DdpFleetArgs) * (size_t)kMaxFleet,
                                                   sizeof(NominalFleetArgs) * (size_t)kMaxFleet, sizeof(TraceFleetArgs) * (size_t)kMaxFleet,
                                                   sizeof(TraceSelectArgs) * (size_t)kMaxFleet,
                                                   sizeof(NominalGainsFleetArgs) * (size_t)kMaxFleet})) == hipSuccess;
  return fb.ready ? &fb : nullptr;
}

// a handle's own one-instance block: the rollout arguments and, for a form with list descriptors, one of them behind
static size_t fleet_one_net_offset() { return align16(sizeof(RolloutArgs)); }
static size_t fleet_one_bytes(bool with_net) { return with_net ? fleet_one_net_offset() + sizeof(FleetGlbNet) : sizeof(RolloutArgs); }

int fleet_prepare(mppi_handle *h, bool with_net)
{
  if (h->fleet_one && h->fleet_one->slot >= fleet_one_bytes(with_net)) return MPPI_OK;
  HIPCHK(h, ensure_device(h->cfg.device));
  ArgBlock *b = new (std::nothrow) ArgBlock;
  if (!b) return fail(h, MPPI_ERR_HIP, "out of memory");
  const hipError_t e = arg_block_create(*b, fleet_one_bytes(with_net));
  if (e != hipSuccess) {
    delete b;
    return fail(h, MPPI_ERR_HIP, "fleet form: argument block", e);
  }
  if (h->fleet_one) {  // the block of another fleet form, too small for the descriptor: nothing of it is in flight any more
    HIPCHK(h, hipStreamSynchronize(h->stream));
    arg_block_destroy(*h->fleet_one);
    delete h->fleet_one;
  }
  h->fleet_one = b;
  return MPPI_OK;
}

// a handle of a fleet form solved alone: the fleet's kernel with one instance, its argument block sent on the handle's own stream
hipError_t launch_rollout_fleet_one(mppi_handle *h, const RolloutArgs &a)
{
  if (!h->fleet_one || !form_desc(h->forced).fleet) return hipErrorInvalidValue;
  unsigned char *host = nullptr;
  if (hipError_t e = arg_block_stage(*h->fleet_one, &host); e != hipSuccess) return e;
  const FormDesc &d = form_desc(h->forced);
  memcpy(host, &a, sizeof(RolloutArgs));
  if (d.fleet_net) {
    const FleetGlbNet net = d.fleet_net(h);
    memcpy(host + fleet_one_net_offset(), &net, sizeof(net));
  }
  if (hipError_t e = arg_block_send(*h->fleet_one, fleet_one_bytes(d.fleet_net != nullptr), h->stream); e != hipSuccess) return e;
  mppi_handle *const hs[1] = {h};
  return d.fleet(hs, &a, reinterpret_cast<const RolloutArgs *>(h->fleet_one->d), reinterpret_cast<const FleetGlbNet *>(h->fleet_one->d + fleet_one_net_offset()), 1,
                 h->stream);
}

void fill_cost_args(const mppi_handle *h, CostArgs &c)
{
  const mppi_cost_params &p = h->cost;
  c.desired_speed = p.desired_speed;
  c.speed_coeff = p.speed_coeff;
  c.track_coeff = p.track_coeff;
  c.max_slip_ang = p.max_slip_ang;
  c.slip_penalty = p.slip_penalty;
  c.track_slop = p.track_slop;
  c.crash_coeff = p.crash_coeff;
  c.steering_coeff = p.steering_coeff;
  c.throttle_coeff = p.throttle_coeff;
  c.boundary_threshold = p.boundary_threshold;
  c.crash_cost_discounted = (float)((1.0 - (double)p.discount) * (double)p.crash_coeff);
  c.l1_cost = p.l1_cost ? 1 : 0;
  for (int i = 0; i < 3; i++) {
    c.r_c1[i] = h->r_c1[i];
    c.r_c2[i] = h->r_c2[i];
    c.trs[i] = h->trs[i];
  }
  c.affine = (h->r_c1[2] == 0.0f && h->r_c2[2] == 0.0f && h->trs[2] == 1.0f) ? 1 : 0;
  const float n0 = h->cfg.exploration_std[0], n1 = h->cfg.exploration_std[1];
  const bool nu_ok = std::isfinite(n0) && std::isfinite(n1) && n0 * n0 > 0.0f && n1 * n1 > 0.0f &&
                     std::isfinite(n0 * n0) && std::isfinite(n1 * n1);
  c.need_control_cost = (p.steering_coeff != 0.0f || p.throttle_coeff != 0.0f || !nu_ok) ? 1 : 0;
  c.map_w = h->map_w;
  c.map_h = h->map_h;
  c.map = h->d_map;
}

void fill_rollout_args(const mppi_handle *h, const float *state, float *noise, RolloutArgs &a)
{
  for (int i = 0; i < kStateDim; i++) a.state[i] = state[i];
  a.U = h->d_in;
  a.noise = noise;
  a.costs = h->d_costs;
  const FormDesc &d = form_desc(form_of(h));
  a.wpack = image(h, d.image);
  a.inv_t = h->d_invt;
  a.K = h->K;
  a.T = h->T;
  a.opt_delay = h->cfg.optimization_stride;
  a.k99 = h->k99;
  for (int i = 0; i < 2; i++) {
    a.nu[i] = h->cfg.exploration_std[i];
    a.u_lo[i] = h->u_lo[i];
    a.u_hi[i] = h->u_hi[i];
  }
  a.dt = h->dt;
  a.negate_yaw_der = (h->cfg.negate_yaw_der || d.has(kNegateYaw)) ? 1 : 0;
  a.rng_in = nullptr;
  a.rng_out = nullptr;
  a.inline_noise = 0;
  a.gate = nullptr;
  a.gate_seq = 0;
  a.gate_ticks = 10000000u;  // gated launches: armed_args sets it
  a.min_cost = nullptr;  // tag_min_cost
  a.min_cost_tag = 0;
  // roles 32-34 are waits of the streaming tail kernel (tail_launch): the rollout runs with its defaults
  a.spin_budget = h->fault_wave >= 32 ? 0 : h->spin_budget;
  a.fault_wave = h->fault_wave >= 32 ? 0 : h->fault_wave;
  fill_cost_args(h, a.cost);
}

// Where the tail stage is the streaming kernel (K > 4096) AND the rollout form is one of rollout_multi.hip's (the automatic ones
// beyond 8192 rollouts) beta comes out of the rollout kernel: -0.8 us of the step at K = 16 384, -1.7 at config 4.  With the row /
// m44 forms (every K <= 8192 by default) the same was measured a LOSS (headline 0.0393 -> 0.0403 ms: the device-scope atomic at the end of the
// cost wave costs the rollout kernel 0.6 us, and the tail's own block reduction was never on its critical path) -- not used there.
static unsigned long long *min_cost_keys(const mppi_handle *h)
{
  return (h->use_min_cost && tail_is_stream(h->K) && form_desc(form_of(h)).has(kPublishes)) ? h->d_min_cost : nullptr;
}

int tag_min_cost(mppi_handle *h, RolloutArgs &a, hipStream_t stream)
{
  h->min_cost_tag++;  // also without the keys: whatever an earlier launch left there is not this launch's
  if (h->min_cost_tag == 0xFFFFFFFFu) {  // 4e9 launches on: ~tag has run out -- all keys back to "none", tags from 1 again
    HIPCHK(h, hipMemsetAsync(h->d_min_cost, 0xFF, sizeof(unsigned long long) * kMinCostLines * kMinCostStride, stream));
    h->min_cost_tag = 1;
  }
  a.min_cost = min_cost_keys(h);
  a.min_cost_tag = h->min_cost_tag;
  return MPPI_OK;
}

int launch_rollout(mppi_handle *h, const RolloutArgs &a)
{
  const FormDesc &d = form_desc(form_of(h));
  const hipError_t e = d.launch ? d.launch(h, d, a, h->stream) : hipErrorInvalidValue;
  if (e != hipSuccess) return fail(h, MPPI_ERR_HIP, "rollout launch", e);
  h->launch_instances = 1;
  h->launch_gated = a.gate != nullptr;
  return MPPI_OK;
}

int check_ready(mppi_handle *h)
{
  if (!h) return MPPI_ERR_INVALID;
  if (!h->have_nn) return fail(h, MPPI_ERR_STATE, "mppi_set_nn_params has not been called");
  if (!h->have_map) return fail(h, MPPI_ERR_STATE, "mppi_set_costmap has not been called");
  if (!h->have_cost) return fail(h, MPPI_ERR_STATE, "mppi_set_cost_params has not been called");
  return MPPI_OK;
}

// Stand-alone generator (mppi_generate_noise, and solves with a rollout variant that has no noise wavefront,
// or any variant while prefetched draws are waiting): *buf_out holds the draws of the next solve iteration once
// the handle's stream has passed the wait enqueued here.
int launch_generator(mppi_handle *h, float *dst)
{
  const bool timed = h->gen_time_now && !h->gen_timed;
  if (timed) HIPCHK(h, hipEventRecord(h->ev_gt[0], h->gstream));
  HIPCHK(h, launch_noise(h->d_rng[h->rng_cur], h->d_rng[1 - h->rng_cur], h->d_jump, h->K, h->T, h->noise_L,
                         h->noise_C, dst, h->gstream));
  if (timed) {
    HIPCHK(h, hipEventRecord(h->ev_gt[1], h->gstream));
    h->gen_timed = true;
  }
  h->rng_cur = 1 - h->rng_cur;
  HIPCHK(h, hipEventRecord(h->ev_gen, h->gstream));
  return MPPI_OK;
}

int acquire_noise(mppi_handle *h, float **buf_out)
{
  if (!h->gen_async) {
    // small problems: the generator on the handle's own stream, in front of the rollout.  The two event waits of
    // the asynchronous path cost ~10 us per solve, more than a generator of K T < 2^20 pairs takes
    // (basis-function build, K=2560: 86 -> 92 us per solve with it; config 4, 2.4 M pairs: 355 -> 337 us)
    h->gen_cur = 1 - h->gen_cur;
    float *dst = h->d_gen[h->gen_cur];
    HIPCHK(h, launch_noise(h->d_rng[h->rng_cur], h->d_rng[1 - h->rng_cur], h->d_jump, h->K, h->T, h->noise_L,
                           h->noise_C, dst, h->stream));
    h->rng_cur = 1 - h->rng_cur;
    *buf_out = dst;
    return MPPI_OK;
  }
  if (!h->prefetch_valid) {
    // generate now: after everything enqueued on the handle's stream so far (the buffer may still be read by an
    // earlier iteration's tail kernel, the generator states may have been written by an in-kernel generator)
    HIPCHK(h, hipEventRecord(h->ev_s1, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->gstream, h->ev_s1, 0));
    int rc = launch_generator(h, h->d_gen[1 - h->gen_cur]);
    if (rc) return rc;
  }
  h->prefetch_valid = false;
  h->gen_cur = 1 - h->gen_cur;
  HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_gen, 0));
  *buf_out = h->d_gen[h->gen_cur];
  return MPPI_OK;
}

// Does the generator kernel of the NEXT solve start at once, beside this solve's rollout (on the lowest-priority stream: it
// gets what the dynamics waves leave), or behind it, beside the tail kernel?  Beside, while it does not compete with rollout
// workgroups that still wait for a slot (profiles/r05_p_generator_beside_rollout.txt, steps in ms, behind -> beside):
//   one dynamics wave per SIMD (K <= 16 384): round 3's measurement (config 4 0.317 -> 0.309);
//   64-wide nets at any K: K = 24 576 / T = 150 0.5245 -> 0.5090, K = 32 768 0.3684 -> 0.3584, K = 65 536 0.7121 -> 0.7014 (their
//     matrix-instruction chains leave the bubbles even with four rounds of workgroups);
//   32-wide nets while every rollout workgroup is resident at once (two per CU: K <= 32 768): K = 24 576 0.1709 -> 0.1551,
//     K = 32 768 0.1757 -> 0.1610, 6-32x4-4 K = 32 768 0.3146 -> 0.2985; at K = 65 536 (two rounds) the generator's workgroups
//     take the slots the second round waits for: 0.3112 -> 0.3639, so there it starts when the rollout ends.
// MPPI_GEN_BESIDE=0 / 1 (tools only) forces either.
bool gen_beside_rollout(const mppi_handle *h)
{
  static const int forced = [] { const char *e = getenv("MPPI_GEN_BESIDE"); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }();
  if (forced >= 0) return forced == 1;
  if (h->K / kRolloutsPerWave <= h->num_simds) return true;
  if (h->hidden >= 64) return true;
  return h->K / 64 <= 2 * (h->num_simds / 4);
}

// The next solve's draws, requested right after this solve's rollout went out: they start when that rollout
// ends (ev_s1) and run beside the weights / tail kernels.  Their target is the buffer of the solve BEFORE this
// one, which the host has collected.  Only for single-iteration solves of a generator-kernel form.
int prefetch_noise(mppi_handle *h)
{
  // INVARIANT the target buffer relies on: d_gen[1 - gen_cur] holds the applied controls of the solve BEFORE the
  // one just enqueued; its readers were that solve's tail kernel -- every row workgroup published its row after
  // reading it, and the host has seen all rows (wait_pending at the top of enqueue_solve) -- and calls that
  // synchronise the stream themselves (mppi_get_applied_controls, mppi_rollout_only).  No device-side ordering
  // against h->stream is needed as long as no solve is pending here; a reader that does not synchronise would
  // have to be ordered explicitly (an event after the tail kernel, waited for by gstream).
  if (h->pending) return fail(h, MPPI_ERR_STATE, "prefetch with a solve pending");
  // beside the rollout or behind it: gen_beside_rollout
  if (!gen_beside_rollout(h)) HIPCHK(h, hipStreamWaitEvent(h->gstream, h->ev_s1, 0));
  int rc = launch_generator(h, h->d_gen[1 - h->gen_cur]);
  if (rc) return rc;
  h->prefetch_valid = true;
  return MPPI_OK;
}

// the sequence number of the next solve: above every number a solve on this handle published under -- the last one, and a
// solve called off (solve_ahead_disarm) whose tail kernel still publishes (poisoned) under its own
static unsigned next_seq(const mppi_handle *h)
{
  return (h->seq_floor - h->seq < 0x80000000u ? h->seq_floor : h->seq) + 1;
}

// the tag of the next tail launch's granules (many-chunk solves; never 0)
static void next_tail_epoch(mppi_handle *h)
{
  if (++h->tail_epoch == 0) h->tail_epoch = 1;
}

// the rollout kernel's noise wavefront draws eps itself, from the generator state the handle is at, and leaves the next one
static void use_inline_noise(mppi_handle *h, RolloutArgs &a)
{
  a.inline_noise = 1;
  a.rng_in = h->d_rng[h->rng_cur];
  a.rng_out = h->d_rng[1 - h->rng_cur];
  h->rng_cur = 1 - h->rng_cur;
}

// the first batched launch after work on the handle's own streams: that work finishes first
static int hand_over(mppi_handle *h, hipStream_t batch)
{
  if (h->order_stream == batch) return MPPI_OK;
  hipError_t e = hipStreamSynchronize(work_stream(h));
  if (e == hipSuccess) e = hipStreamSynchronize(h->gstream);
  if (e != hipSuccess) return fail(h, MPPI_ERR_HIP, "stream hand-over to the batch stream", e);
  h->order_stream = batch;
  return MPPI_OK;
}

int upload_controls_if_dirty(mppi_handle *h, hipStream_t stream)
{
  if (!h->u_dirty) return MPPI_OK;
  memcpy(h->h_in, h->U.data(), sizeof(float) * 2 * (size_t)h->T);
  memcpy(h->h_in + 2 * h->T, h->hist.data(), sizeof(float) * 4);
  HIPCHK(h, hipMemcpyAsync(h->d_in, h->h_in, sizeof(float) * (2 * (size_t)h->T + 4), hipMemcpyHostToDevice,
                           stream));
  h->u_dirty = false;
  return MPPI_OK;
}

// -DMPPI_HOSTPROF (a diagnostic build: tools/build_variant.sh): where the host's microseconds of a solve go, averaged per call
// and printed to stderr every 1000 calls of a driver.  HP_CLOCK(t) starts a clock, HP(stage, t) adds the time since t (or since
// the last HP on t) to a stage, HP_CALL(first) counts a call of the driver whose stages begin at `first` and prints them.  The
// default build contains none of it.
#ifdef MPPI_HOSTPROF
enum HpStage { kHpEntry, kHpRollout, kHpTail, kHpSmoothed,                           // enqueue_solve per iteration; wait_pending
               kHpDecide, kHpStream, kHpWait, kHpArgs, kHpPairRollout, kHpPairTail,  // a batch that shares one rollout launch
               kHpStages };
static const char *const hp_name[kHpStages] = {"entry->launch", "rollout launch", "tail launch", "poll->smoothed", "decide",
                                               "device + stream", "wait_pending", "upload+args", "rollout launch", "tail launch"};
static double hp_acc[kHpStages] = {0};
static long hp_calls[kHpStages] = {0};  // [first stage of a driver]
#define HP_CLOCK(t) auto t = std::chrono::steady_clock::now()
#define HP(stage, t) do { const auto n__ = std::chrono::steady_clock::now(); hp_acc[stage] += std::chrono::duration<double, std::micro>(n__ - (t)).count(); (t) = n__; } while (0)
#define HP_CALL(first) do { if (++hp_calls[first] % 1000 == 0) hp_print(first); } while (0)
static void hp_print(int first)
{
  // (the first batched call creates the device's batch stream, ~3 ms: read the averages over many calls with that in mind)
  fprintf(stderr, "hostprof %s (us per call, %ld calls):", first == kHpDecide ? "batch" : "solve", hp_calls[first]);
  for (int i = first; i < (first == kHpDecide ? kHpStages : kHpDecide); i++) fprintf(stderr, " %s %.2f |", hp_name[i], hp_acc[i] / hp_calls[first]);
  fprintf(stderr, "\n");
}
#else
#define HP_CLOCK(t) do { } while (0)
#define HP(stage, t) do { } while (0)
#define HP_CALL(first) do { } while (0)
#endif

// savitskyGolay (mppi_controller.cu:468-499) on the host, the same operations in the same order as the tail
// kernel applies to the device copy (this file is compiled with -ffp-contract=off):
// X = [hist0, hist1, U_0 .. U_{T-1}, U_{T-1}, U_{T-1}], U_i = sum_m f_m X_{i+m}.  Row t of the unsmoothed
// sequence is (src[stride t], src[stride t + off1]); the result goes to h->U.
void savgol_host(mppi_handle *h, const float *src, int stride, int off1)
{
  const int T = h->T;
  std::vector<float> &X = h->sg_buf;
  X.resize((size_t)(T + 4) * 2);
  for (int j = 0; j < 4; j++) X[j] = h->hist[j];
  for (int t = 0; t < T; t++) {
    X[(t + 2) * 2 + 0] = src[stride * t + 0];
    X[(t + 2) * 2 + 1] = src[stride * t + off1];
  }
  for (int r = T + 2; r < T + 4; r++)
    for (int j = 0; j < 2; j++) X[r * 2 + j] = X[(T + 1) * 2 + j];
  const float f0 = -3.0f / 35.0f, f1 = 12.0f / 35.0f, f2 = 17.0f / 35.0f;
  for (int i = 0; i < 2 * T; i++) {
    float acc = f0 * X[i];
    float p = f1 * X[i + 2];
    acc = acc + p;
    p = f2 * X[i + 4];
    acc = acc + p;
    p = f1 * X[i + 6];
    acc = acc + p;
    p = f0 * X[i + 8];
    acc = acc + p;
    h->U[i] = acc;
  }
}

// Waits for the pending solve: polls the sequence number the tail kernel publishes (system-scope
// release) in the host-mapped result block; no stream synchronise on the fast path.
// A solve whose wait ran out of time (mppi_set_wait_timeout) leaves the handle "timed out": nothing waits for that solve
// again -- every later entry returns at once -- until its device work has drained (one hipStreamQuery per call, no
// blocking); then the handle works again from the host's copies of U / hist, which the failed solve never touched.
int recover_timed_out(mppi_handle *h)
{
  if (!h->timed_out) return MPPI_OK;
  const hipError_t q = hipStreamQuery(work_stream(h));
  if (q == hipErrorNotReady) return fail(h, MPPI_ERR_HIP, "an earlier solve timed out and its device work has not finished yet");
  if (q != hipSuccess) return fail(h, MPPI_ERR_HIP, "an earlier solve timed out; hipStreamQuery", q);
  h->timed_out = false;
  return MPPI_OK;
}

int wait_pending(mppi_handle *h)
{
  if (!h->pending) return recover_timed_out(h);  // nothing to wait for; a lost solve's device work must have drained
  // The tail kernel writes T+2 entries of 16 B into host-mapped memory -- row t: [u0, seq, u1, seq], then
  // [beta, seq, eta, seq] and [trajectory cost, seq, 0, seq] -- each as one store.  An entry is complete
  // once words 1 and 3 carry this solve's sequence number (either 8-byte half may land first); the solve
  // is complete for the host once every entry is.
  const volatile unsigned *words = reinterpret_cast<const volatile unsigned *>(h->h_res);
  const int n_entries = h->T + 2;
  const auto t0 = std::chrono::steady_clock::now();
  unsigned long spins = 0;
  double next_query_s = 0.01;  // the stream is asked whether it has drained every 10 ms of waiting, never on the fast path
  int next = 0;  // entries [0, next) have been seen with the sequence number
  // the host's copies are all that can be trusted after a failed wait: the next solve uploads them again, no slid copy is
  // offered, and nothing waits for this solve a second time (recover_timed_out)
  auto give_up = [&](const char *what, bool timed_out) {
    h->pending = false;
    h->pending_armed = false;
    h->pending_timed = false;
    h->u_dirty = true;
    h->slid_valid = false;
    h->timed_out = timed_out;
    h->no_result = true;  // until the next solve completes: the result getters refuse
    return fail(h, MPPI_ERR_HIP, what);
  };
  for (;;) {
    while (next < n_entries && __atomic_load_n(words + 4 * next + 1, __ATOMIC_ACQUIRE) == h->seq &&
           __atomic_load_n(words + 4 * next + 3, __ATOMIC_ACQUIRE) == h->seq)
      next++;
    if (next == n_entries) break;
    __builtin_ia32_pause();
    if ((++spins & 0xFF) == 0) {  // the clock every 256 polls (a vDSO read, ~20 ns): the limit holds to microseconds
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (el > h->wait_timeout_s) return give_up("timed out waiting for the solve", true);
      if (el > next_query_s) {
        next_query_s = el + 0.01;
        if (hipStreamQuery(work_stream(h)) == hipSuccess && (__atomic_load_n(words + 4 * next + 1, __ATOMIC_ACQUIRE) != h->seq ||
                                                        __atomic_load_n(words + 4 * next + 3, __ATOMIC_ACQUIRE) != h->seq))
          return give_up("solve finished without publishing its result block", false);
      }
    }
  }
  HP_CLOCK(hp_t);
  h->pending = false;
  h->no_result = false;
  h->baseline = h->h_res[4 * h->T + 0];
  h->eta = h->h_res[4 * h->T + 2];
  h->traj_cost = h->h_res[4 * (h->T + 1) + 0];
  // The result block is checked BEFORE the host's copies of U take it: a poisoned or failed solve never reaches h->U (the next
  // solve starts from the sequence the host held; the device copy, which that solve's tail smoothed, is not trusted).
  // The minimum-cost rollout has weight 1 and costs are capped (never NaN), so eta >= 1 always.
  // Anything else means a rollout wavefront gave up on a hand-over (its spin budget) and poisoned
  // its costs: report it instead of returning a NaN control sequence.
  const bool eta_ok = h->eta >= 1.0f;
  bool rows_ok = true;
  if (eta_ok && (tail_is_stream(h->K) || h->pending_armed)) {
    // the one-launch tail of many-chunk solves: a row workgroup whose wait for another workgroup's granule ran out of time
    // published NaN in place of what it waited for; a gated solve: its rows, whatever its tail
    rows_ok = std::isfinite(h->traj_cost);
    for (int t = 0; t < h->T && rows_ok; t++) rows_ok = std::isfinite(h->h_res[4 * t]) && std::isfinite(h->h_res[4 * t + 2]);
  }
  h->pending_armed = false;
  if (!eta_ok || !rows_ok) {
    h->u_dirty = true;
    h->slid_valid = false;
    return fail(h, MPPI_ERR_HIP, !eta_ok ? "solve produced a non-finite normaliser (device hand-over failed)"
                                         : "solve produced non-finite controls (device hand-over failed)");
  }
  savgol_host(h, h->h_res, 4, 2);  // rows [u0, seq, u1, seq] of the result block
  HP(kHpSmoothed, hp_t);
  if (h->pending_timed) {
    h->pending_timed = false;
    for (size_t it = 0; it < h->ev.size(); it++) {
      HIPCHK(h, hipEventSynchronize(h->ev[it].e[3]));
      float ms[3] = {0, 0, 0};
      for (int i = 0; i < 3; i++) (void)hipEventElapsedTime(&ms[i], h->ev[it].e[i], h->ev[it].e[i + 1]);
      // the rollout stage: the kernel's own dispatch stamps where the runtime delivered them
      float kms = 0.0f;
      if (hipEventElapsedTime(&kms, h->ev[it].e[4], h->ev[it].e[5]) == hipSuccess && kms > 0.0f) {
        ms[1] = kms;
      }
      h->acc.noise_ms += ms[0];
      h->acc.rollout_ms += ms[1];
      h->acc.reduction_ms += ms[2];
      h->acc.total_ms += ms[0] + ms[1] + ms[2];
    }
    if (h->gen_timed) {  // the generator launch enqueued during this solve (on gstream, beside the rollout / tail)
      h->gen_timed = false;
      float gms = 0.0f;
      HIPCHK(h, hipEventSynchronize(h->ev_gt[1]));
      if (hipEventElapsedTime(&gms, h->ev_gt[0], h->ev_gt[1]) == hipSuccess && gms > 0.0f) h->acc.noise_ms += gms;
    }
    h->acc.n_solves += 1;
  }
  return MPPI_OK;
}

// the tail kernel of the last iteration leaves [U | hist] slid by the optimization stride in the other buffer
bool wants_slid_copy(const mppi_handle *h)
{
  return h->cfg.optimization_stride >= 1 && h->cfg.optimization_stride < h->T;
}

TailLaunch tail_launch(const mppi_handle *h, const float *V, bool last)
{
  TailLaunch l;
  l.costs = h->d_costs; l.V = V; l.U = h->d_in; l.hist = h->d_in + 2 * h->T; l.w = h->d_w; l.scal = h->d_scal;
  l.res = h->d_res_map; l.counter = h->d_counter;
  l.K = h->K; l.T = h->T; l.gamma = h->cfg.gamma; l.last_iter = last ? 1 : 0; l.seq = h->seq;
  l.slid = (last && wants_slid_copy(h)) ? h->d_in_buf[1 - h->in_cur] : nullptr;
  l.slide_stride = h->cfg.optimization_stride;
  l.init0 = h->cfg.init_control[0]; l.init1 = h->cfg.init_control[1];
  // the one-launch streaming tail (K > 4096): granule buffers, this launch's tag (the caller advanced it), wait deadline; the
  // tests' fault roles 32-34 shorten the deadline to spin_budget x 1 us
  l.ug = h->d_ug;
  l.gx = h->d_gx; l.gpart = reinterpret_cast<unsigned long long *>(h->d_part);
  l.epoch = h->tail_epoch;
  l.fault = h->fault_wave >= 32 ? h->fault_wave : 0;
  l.poll_ticks = (l.fault && h->spin_budget > 0) ? (unsigned)h->spin_budget * 100u : h->tail_poll_ticks;
  l.min_cost = min_cost_keys(h);
  l.min_cost_tag = h->min_cost_tag;
  return l;
}

// ---- the phases of a solve -------------------------------------------------------------------------------------------------
// "Enqueue a solve for the handles hs[0 .. n) on stream S" in the order every driver below runs it: collect; begin_solves; per
// iteration solve_step for every handle, then the driver's own launches; finish_solves.  A batched driver answers every failure
// after begin_solves with distrust.  n = 1 drivers pass one stack RolloutArgs / TailLaunch; only the fleet driver owns arrays.

// Whatever can fail without moving a handle fails here: every handle's timed-out solve has drained, its pending solve is
// collected.  (Nothing is checked about explicit noise: see explicit_iters, abi_internal.hpp.)
static int collect(mppi_handle *const *hs, int n)
{
  for (int i = 0; i < n; i++) {
    int rc = recover_timed_out(hs[i]);
    if (rc == MPPI_OK) rc = wait_pending(hs[i]);  // finish a previous asynchronous solve first
    if (rc) return rc;
  }
  return MPPI_OK;
}

// From here on handles change (sequence numbers, generator buffers, the slid copy's validity).  batched: S is the device's batch
// stream, and a handle's work on its own streams finishes first.
static int begin_solves(mppi_handle *const *hs, int n, hipStream_t S, bool batched)
{
  for (int i = 0; i < n; i++) {
    mppi_handle *h = hs[i];
    int rc = batched ? hand_over(h, S) : MPPI_OK;
    if (rc == MPPI_OK) rc = upload_controls_if_dirty(h, S);
    if (rc) return rc;
    h->seq = next_seq(h);
    forget_solve_state(h);
  }
  return MPPI_OK;
}

// A failure between begin_solves and finish_solves of a batched solve leaves every handle of the batch in the state "nothing on
// the device can be trusted": the host copies of U / hist are uploaded again by the next solve, no slid copy is offered to
// mppi_slide_control_seq, nothing is pending.
static int distrust(mppi_handle *const *hs, int n, int rc)
{
  for (int i = 0; i < n; i++) {
    hs[i]->slid_valid = false;
    hs[i]->u_dirty = true;
    hs[i]->pending = false;
  }
  return rc;
}

// Where the eps of an iteration come from.  The explicit buffer (mppi_set_noise) goes first on every path; without one
//   Single: draws already prefetched > the rollout kernel's own noise wavefront > the generator kernel, now (acquire_noise);
//   Pair:   the rollout kernel's own noise wavefront (every batched kernel has one; batch_together admits no prefetched draws);
//   Fleet:  the fleet's one generator launch, from the descriptor filled here -- the handle's generator stream and buffers move
//           exactly as acquire_noise moves them for its own solve.
enum class Eps { Single, Pair, Fleet };

// *buf: iteration it's eps, which the rollout overwrites with the applied controls (v_buf).  *in_kernel: the caller's rollout
// arguments take use_inline_noise once they are filled.  nd (Fleet only): the handle's generator descriptor; draws nothing
// where the noise is explicit.
static int eps_source(mppi_handle *h, Eps src, int it, float **buf, bool *in_kernel, NoiseFleetDesc *nd)
{
  *in_kernel = false;
  if (src == Eps::Fleet) *nd = NoiseFleetDesc{};
  if (h->explicit_iters > 0) {
    *buf = h->d_noise + (size_t)it * ((size_t)h->K * h->T * 2);
  } else if (src == Eps::Fleet) {
    h->gen_cur = 1 - h->gen_cur;
    *buf = h->d_gen[h->gen_cur];
    *nd = NoiseFleetDesc{h->d_rng[h->rng_cur], h->d_rng[1 - h->rng_cur], h->d_jump, *buf, h->K, h->T, h->noise_L, h->noise_C};
    h->rng_cur = 1 - h->rng_cur;
  } else if (src == Eps::Pair || (!h->prefetch_valid && has_noise_wave(h))) {
    *in_kernel = true;
    *buf = h->d_gen[h->gen_cur];
  } else if (int rc = acquire_noise(h, buf)) {
    return rc;
  }
  h->v_buf = *buf;
  return MPPI_OK;
}

// One handle's share of iteration `it`: its eps, and the rollout and tail arguments of the launches the driver makes on S.
// (The tail's epoch advances on every path; only the streaming tail, K > 4096, reads it, and a batch never runs that tail.)
static int solve_step(mppi_handle *h, const float *state, int it, bool last, hipStream_t S, Eps src, RolloutArgs &a, TailLaunch &l,
                      NoiseFleetDesc *nd)
{
  float *noise = nullptr;
  bool in_kernel = false;
  int rc = eps_source(h, src, it, &noise, &in_kernel, nd);
  if (rc) return rc;
  fill_rollout_args(h, state, noise, a);
  rc = tag_min_cost(h, a, S);
  if (rc) return rc;
  if (in_kernel) use_inline_noise(h, a);
  next_tail_epoch(h);
  l = tail_launch(h, noise, last);
  return MPPI_OK;
}

// Every launch of the solve is on its stream.  (The slid copy the last tail leaves becomes valid here, not in solve_step: a
// solve whose launches failed offers none.)
static void finish_solves(mppi_handle *const *hs, const float *states, int n, bool timed)
{
  for (int i = 0; i < n; i++) {
    mppi_handle *h = hs[i];
    h->explicit_iters = 0;
    h->slid_valid = wants_slid_copy(h);
    h->pending = true;
    note_solve_state(h, states + (size_t)MPPI_STATE_DIM * i, true);
    h->pending_timed = timed;
  }
}

// current device, then the batch stream of h0's device (looked up once per handle)
static int use_batch_stream(mppi_handle *h0, hipStream_t *S)
{
  HIPCHK(h0, ensure_device(h0->cfg.device));
  if (!h0->batch_s) h0->batch_s = batch_stream(h0->cfg.device);
  *S = h0->batch_s;
  return *S ? MPPI_OK : fail(h0, MPPI_ERR_HIP, "no batch stream");
}

static bool arm_usable(const mppi_handle *h);
static int open_armed(mppi_handle *h, const float *state);

// One handle on its own stream: launch_rollout + launch_solve_tail per iteration, with the stage events, the capture copies and
// the prefetch of the next solve's draws behind the rollout.
int enqueue_solve(mppi_handle *h, const float *state)
{
  HP_CLOCK(hp_t);
  int rc = check_ready(h);
  if (rc) return rc;
  if (!state) return fail(h, MPPI_ERR_INVALID, "state is NULL");
  rc = recover_timed_out(h);  // (an armed solve of a handle that has not drained is left alone)
  if (rc) return rc;
  rc = collect(&h, 1);
  if (h->armed) {
    // armed (mppi_arm): this call opens the gate of the solve already enqueued -- unless the previous solve failed, the armed
    // solve belongs to a batch, or its deadline has passed: then it is called off and this solve runs as if it never was
    if (rc == MPPI_OK && h->arm_n == 0 && arm_usable(h)) return open_armed(h, state);
    const int drc = solve_ahead_disarm(h);
    if (rc == MPPI_OK) rc = drc;
  }
  if (rc) return rc;
  const int K = h->K, T = h->T, iters = h->cfg.num_iters;
  OWN(h);
  rc = begin_solves(&h, 1, h->stream, false);
  if (rc) return rc;
  const bool timed = h->timing && (h->timing_count++ % (unsigned)h->timing_every) == 0;
  const bool explicit_noise = h->explicit_iters > 0;
  for (int it = 0; it < iters; it++) {
    Events *ev = timed ? &h->ev[it] : nullptr;
    if (ev) HIPCHK(h, hipEventRecord(ev->e[0], h->stream));
    const bool last = (it == iters - 1);
    RolloutArgs a;
    TailLaunch l;
    rc = solve_step(h, state, it, last, h->stream, Eps::Single, a, l, nullptr);
    if (rc) return rc;
    if (ev) HIPCHK(h, hipEventRecord(ev->e[1], h->stream));  // behind the generator, where this iteration waited for one
    HP(kHpEntry, hp_t);  // entry -> before the rollout launch
    if (ev) { tl_kernel_start = ev->e[4]; tl_kernel_stop = ev->e[5]; }
    rc = launch_rollout(h, a);
    tl_kernel_start = tl_kernel_stop = nullptr;
    if (rc) return rc;
    HP(kHpRollout, hp_t);  // the rollout launch call
    const bool prefetch = h->gen_async && iters == 1 && !explicit_noise && !has_noise_wave(h) && !h->prefetch_valid;
    if (prefetch) HIPCHK(h, hipEventRecord(h->ev_s1, h->stream));  // the generator starts when this rollout ends
    if (ev) HIPCHK(h, hipEventRecord(ev->e[2], h->stream));
    HIPCHK(h, launch_solve_tail(l, h->stream));
    if (h->capture) {  // test hook: what this iteration left (the last iteration's raw U is in the result block)
      float *c = h->d_cap + (size_t)it * (2 * (size_t)T + K);
      if (!last) HIPCHK(h, hipMemcpyAsync(c, h->d_in, sizeof(float) * 2 * (size_t)T, hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(c + 2 * (size_t)T, h->d_costs, sizeof(float) * (size_t)K, hipMemcpyDeviceToDevice, h->stream));
    }
    if (prefetch) {
      h->gen_time_now = timed;  // only the prefetch launch: a generator the stream waits for sits between e[0] and e[1]
      rc = prefetch_noise(h);
      h->gen_time_now = false;
      if (rc) return rc;
    }
    HP(kHpTail, hp_t);  // the tail launch call
    HP_CALL(kHpEntry);
    if (ev) HIPCHK(h, hipEventRecord(ev->e[3], h->stream));
  }
  finish_solves(&h, state, 1, timed);
  h->cap_valid = h->capture;
  h->cap_explicit = explicit_noise;
  return MPPI_OK;
}

// ---- solve-ahead (mppi_arm, mppi_control_ticks) ----------------------------------------------------------------------------
// The launches of a solve -- 2.8 us of launch call and 1.5 us of dispatch for the rollout kernel alone, on the step's critical
// path between "result i on the host" and "first instruction of rollout i+1" -- are made one solve AHEAD, while the host would
// otherwise only poll for result i: mppi_arm enqueues the handle's NEXT solve now, gated, behind a pending solve or on an idle
// stream.  Its kernels start, load their weights, draw their first noise and wait; the next mppi_compute_control[_async] does
// not launch: it writes ITS state, the host's U (smoothed and slid, as the reference uploads U_ with every computeControl,
// mppi_controller.cu:608-610) and hist into the gate block and opens the gate.  The solve computes nothing from its inputs before
// the host holds result i.  tools/ub/gate_ub.hip (profiles/r05_c_gate_ub.txt): 46.3 -> 43.0 us per step for stand-in kernels of
// the headline's length with the gate in device memory written through the BAR, 44.5 with a host-mapped gate; two streams with
// the next rollout resident beside the tail: 54 (the cross-stream events cost more than the launches they hide).
// mppi_control_ticks (chained ticks) is a loop over the pair in which every armed solve but the last has a publish-only tail: no
// workgroup smooths a device copy nobody reads, the kernel ends 2.5 us earlier, and the next rollout starts when it ends.
// Results are bit for bit those of the same calls without mppi_arm.  What the armed solve changes before its gate opens is all
// undone by solve_ahead_disarm: its costs / weights go to the second pair of vectors, its applied controls to the generator buffer
// nobody reads, its generator draw (kind 1: the rng_cur flip; kind 2: the prefetched draws, regenerated) is put back, and the
// sequence number it publishes under is never used again.  The device copy of [U | hist] is not kept up while armed (u_dirty:
// slides are the host's alone); the armed tail rewrites both buffers (a publish-only one neither), and the gate's opening points
// d_in at the one it smooths into.

// The forms that have a gated rollout and gain from it (one iteration, no stage events, no capture): 1: a latency form with
// riders (kGate: the row forms, the automatic m44 form, the lds44, lds128 and glb44 forms, the basis-function model's bf_row form) and its in-kernel generator; 2: the automatic multi4-tree form with the
// stand-alone generator kernel prefetched on a second stream; 0: none (the basis-function model's other forms among them: no kGate)
static int arm_kind(const mppi_handle *h)
{
  const Form f = form_of(h);
  if (!(h->d_gate != nullptr && wants_slid_copy(h) && h->cfg.num_iters == 1 && !h->timing && !h->capture &&
        h->explicit_iters == 0 && h->fault_wave == 0 && h->have_nn && h->have_map && h->have_cost && !h->timed_out))
    return 0;
  if (form_desc(f).has(kGate) && has_noise_wave(h) && !h->prefetch_valid) return 1;
  // (where the generator kernel runs beside the rollout.  Where it runs behind it -- 32-wide nets at K = 65 536 -- the phase
  // between two rollouts is the generator's own 41 us whatever the launches cost: chained 0.3139, unchained 0.3131 ms)
  if (f == Form::Multi4Tree && h->forced == Form::Auto && !has_noise_wave(h) && h->gen_async && gen_beside_rollout(h)) return 2;
  return 0;
}

// the armed solve's gate block: its nominal sequence and history (the host's copies, smoothed and slid), its state in every
// replica (memcpy: wide stores -- the block is write-combining memory behind the PCIe BAR where gate_bar is set)
static void write_gate_payload(mppi_handle *h, const float *state)
{
  unsigned *g = gate_host(h);
  const int T = h->T;
  memcpy(g + kGateUOffset, h->U.data(), sizeof(float) * 2 * (size_t)T);
  memcpy(g + gate_hist_offset(T), h->hist.data(), sizeof(float) * 4);
  for (int r = 0; r < kGateReplicas; r++) memcpy(g + 16 * r, state, sizeof(float) * kStateDim);
}

// the gate word in every replica; the fences order whatever was written before in front of it and push it out
static void write_gate_word(mppi_handle *h, unsigned word)
{
  unsigned *g = gate_host(h);
  asm volatile("" ::: "memory");
  __builtin_ia32_sfence();
  for (int r = 0; r < kGateReplicas; r++) __atomic_store_n(g + 16 * r + 7, word, __ATOMIC_RELAXED);
  __builtin_ia32_sfence();
}

// max_wait_s in 100 MHz ticks; the host opens the gate only inside a margin of that (the kernels' clock starts when they do,
// which is after the arming call): a gate opened in time is never one the kernels have given up on
static unsigned arm_ticks(double max_wait_s) { return (unsigned)(max_wait_s * 1e8); }
static std::chrono::steady_clock::time_point arm_deadline(double max_wait_s)
{
  const double open_s = 0.9 * max_wait_s - 50e-6;
  return std::chrono::steady_clock::now() + std::chrono::nanoseconds((long long)((open_s > 0.0 ? open_s : 0.0) * 1e9));
}

// the armed solve's rollout and tail arguments (state: from the gate block)
static void armed_args(mppi_handle *h, float *noise, RolloutArgs &a, TailLaunch &l, double max_wait_s)
{
  static const float no_state[kStateDim] = {0, 0, 0, 0, 0, 0, 0};
  fill_rollout_args(h, no_state, noise, a);
  a.costs = h->d_costs_alt;
  a.U = reinterpret_cast<const float *>(gate_dev(h)) + kGateUOffset;
  a.gate = gate_dev(h);
  a.gate_seq = h->arm_seq;
  a.gate_ticks = arm_ticks(max_wait_s);
  l = tail_launch(h, noise, true);
  l.costs = h->d_costs_alt;
  l.w = h->d_w_alt;
  l.seq = h->arm_seq;
  l.hist = reinterpret_cast<const float *>(gate_dev(h)) + gate_hist_offset(h->T);
  l.U = h->d_in;
  l.hist_out = h->d_in + 2 * h->T;
  l.slid = h->d_in_buf[1 - h->in_cur];
}

// the handle's bookkeeping once its armed solve is on a stream
static void mark_armed(mppi_handle *h, int kind, float *vbuf, hipStream_t stream, double max_wait_s, bool publish_only)
{
  h->armed = kind;
  h->arm_in = h->in_cur;
  h->arm_vbuf = vbuf;
  h->arm_stream = stream;
  h->arm_until = arm_deadline(max_wait_s);
  h->arm_n = 0;
  h->arm_publish_only = publish_only;
  h->u_dirty = true;  // slides until the gate opens are the host's alone (a device slide would queue behind the gated kernel)
  h->slid_valid = false;
}

// One handle's armed solve, everything but its launches on `stream` (mppi_arm, mppi_arm_batch, the chained ticks).  Two facts
// only the chained ticks set: publish_only -- the tail publishes the result and leaves the device copy alone (every armed solve of
// a run but the last); mark -- ev_arm in front of the solve, for the result getters while armed (none runs inside the ticks).
static int arm_handle(mppi_handle *h, int kind, hipStream_t stream, double max_wait_s, bool publish_only, bool mark,
                      RolloutArgs &a, TailLaunch &l)
{
  h->arm_seq = next_seq(h);
  h->gate_blk ^= 1;  // this solve's gate block; the pending solve's tail may still read its own
  float *noise = h->d_gen[1 - h->gen_cur];  // kind 1: the in-kernel generator's applied controls go to the buffer nobody reads
  if (kind == 2) {
    // the draws prefetched for this solve (or, if none are, generated now behind the stream's work); solve_ahead_disarm puts
    // them back
    int rc = acquire_noise(h, &noise);
    if (rc) return rc;
  }
  if (mark) HIPCHK(h, hipEventRecord(h->ev_arm, stream));
  armed_args(h, noise, a, l, max_wait_s);
  int rc = tag_min_cost(h, a, stream);
  if (rc) return rc;
  l.min_cost_tag = h->min_cost_tag;
  if (publish_only) {
    l.no_device_copy = 1;
    l.slid = nullptr;
  }
  if (kind == 1) use_inline_noise(h, a);
  next_tail_epoch(h);
  l.epoch = h->tail_epoch;
  // from here on the handle is armed (a launch error is called off like any armed solve)
  mark_armed(h, kind, noise, stream, max_wait_s, publish_only);
  return MPPI_OK;
}

static int arm_one(mppi_handle *h, double max_wait_s, bool publish_only, bool mark)
{
  const int kind = arm_kind(h);
  if (!kind) return fail(h, MPPI_ERR_UNSUPPORTED, "this handle's form / configuration has no gated form (mppi_arm)");
  OWN(h);  // behind a pending batched solve: the batch stream hands over first (as a solve on the handle's own stream does)
  RolloutArgs a;
  TailLaunch l;
  int rc = arm_handle(h, kind, h->stream, max_wait_s, publish_only, mark, a, l);
  if (rc) return rc;
  rc = launch_rollout(h, a);
  if (rc == MPPI_OK) {
    const hipError_t e = launch_solve_tail(l, h->stream);
    if (e != hipSuccess) rc = fail(h, MPPI_ERR_HIP, "armed tail launch", e);
  }
  if (rc) (void)solve_ahead_disarm(h);
  return rc;
}

// the gate of one armed handle is opened with the cancel bit; its generator stream goes back to where it was
static int disarm_one(mppi_handle *h)
{
  if (!h->armed) return MPPI_OK;
  const int kind = h->armed;
  h->armed = 0;
  h->arm_n = 0;
  write_gate_word(h, h->arm_seq | kGateCancel);
  // its tail publishes (poisoned) under arm_seq and rewrites both device copies of [U | hist]
  h->seq_floor = h->arm_seq;
  h->u_dirty = true;
  h->slid_valid = false;
  h->order_stream = h->arm_stream;
  if (kind == 1) {
    h->rng_cur = 1 - h->rng_cur;  // the called-off kernel read rng_in and wrote the other buffer: the stream is where it was
    return MPPI_OK;
  }
  // kind 2: its draws were consumed (and the called-off kernel may write its applied controls over them): drawn again from the
  // generator state they came from, into the same buffer, once the called-off solve has ended -- as a prefetch
  HIPCHK(h, ensure_device(h->cfg.device));
  h->gen_cur = 1 - h->gen_cur;
  h->rng_cur = 1 - h->rng_cur;
  HIPCHK(h, hipEventRecord(h->ev_s1, h->arm_stream));
  HIPCHK(h, hipStreamWaitEvent(h->gstream, h->ev_s1, 0));
  int rc = launch_generator(h, h->d_gen[1 - h->gen_cur]);
  if (rc) return rc;
  h->prefetch_valid = true;
  return MPPI_OK;
}

int solve_ahead_disarm(mppi_handle *h)
{
  if (!h || !h->armed) return MPPI_OK;
  if (h->arm_n > 0) {  // armed in one launch with its partners: the launch is called off for all of them
    mppi_handle *peers[kMaxBatch];
    const int n = h->arm_n;
    for (int i = 0; i < n; i++) peers[i] = h->arm_peers[i];
    int rc = MPPI_OK;
    for (int i = 0; i < n; i++) {
      const int r = disarm_one(peers[i]);
      if (r && !rc) rc = r;
    }
    return rc;
  }
  return disarm_one(h);
}

// may the armed solve's gate still be opened?  Inside the host's deadline, and its tail has not published (a gated kernel that
// gave up -- or was called off -- publishes poisoned rows under its number)
static bool arm_usable(const mppi_handle *h)
{
  if (std::chrono::steady_clock::now() >= h->arm_until) return false;
  const volatile unsigned *words = reinterpret_cast<const volatile unsigned *>(h->h_res);
  const unsigned s1 = __atomic_load_n(words + 1, __ATOMIC_ACQUIRE), s3 = __atomic_load_n(words + 4 * (h->T + 1) + 1, __ATOMIC_ACQUIRE);
  return s1 != h->arm_seq && s3 != h->arm_seq;
}

// the compute call of an armed handle (its previous solve collected): the gate opens with this state; the armed solve becomes the
// pending one
static int open_armed(mppi_handle *h, const float *state)
{
  const int kind = h->armed;
  h->armed = 0;
  h->arm_n = 0;
  h->seq = h->arm_seq;
  note_solve_state(h, state, true);
  write_gate_payload(h, state);
  write_gate_word(h, h->seq);
  h->order_stream = h->arm_stream;
  std::swap(h->d_costs, h->d_costs_alt);
  std::swap(h->d_w, h->d_w_alt);
  h->v_buf = h->arm_vbuf;
  if (kind == 1) h->gen_cur = h->arm_vbuf == h->d_gen[0] ? 0 : 1;
  h->in_cur = h->arm_in;
  h->d_in = h->d_in_buf[h->in_cur];
  // the armed tail smooths into d_in and leaves the slid copy in the other buffer; a publish-only tail neither
  h->u_dirty = h->arm_publish_only;
  h->slid_valid = !h->arm_publish_only;
  if (kind == 2) {
    // the draws of the solve after it, behind the opened gate, NOT at arming: a generator launch that becomes ready together with
    // the gated rollout (both behind the same tail kernel) takes the CUs first and costs its whole stand-alone time (config 4:
    // 0.2651 -> 0.2834 ms, K = 16 384: 0.0978 -> 0.1071; behind the rollout: 0.2837 / 0.1143; lowest stream priority for the
    // generator: 0.2781).  Here it is a few microseconds behind the rollout's start, filling the dynamics waves' bubbles.
    const int rc = prefetch_noise(h);
    if (rc) {
      h->pending = true;
      h->pending_armed = true;
      return rc;
    }
  }
  h->pending = true;
  h->pending_timed = false;
  h->pending_armed = true;
  h->explicit_iters = 0;
  return MPPI_OK;
}

// the rollout of a batch batch_together admits, in one launch on S; gated: every argument block carries its handle's gate block
static hipError_t launch_rollout_batch(mppi_handle *const *hs, int n, const QuadBatchArgs &qb, bool gated, hipStream_t S)
{
  const FormDesc &d = form_desc(form_of(hs[0]));
  const hipError_t e = d.batch.launch ? d.batch.launch(hs[0], d, qb, S) : hipErrorInvalidValue;
  if (e != hipSuccess) return e;
  for (int i = 0; i < n; i++) {
    hs[i]->launch_instances = n;
    hs[i]->launch_gated = gated;
  }
  return hipSuccess;
}

// mppi_arm_batch: one launch for the batch where mppi_compute_control_batch would use one and the form has a gated batched kernel
// (the row forms; the pair of the automatic m44 form, of the lds44 form, of the lds128 form, of the glb44 form and of the bf_row form)
static bool batch_together(mppi_handle *const *hs, int n);
static int arm_together(mppi_handle *const *hs, int n, double max_wait_s)
{
  mppi_handle *h0 = hs[0];
  if (!form_desc(form_of(h0)).has(kGate))
    return fail(h0, MPPI_ERR_UNSUPPORTED, "the batched launch of this form has no gated form");
  for (int i = 0; i < n; i++)
    if (arm_kind(hs[i]) != 1) return fail(hs[i], MPPI_ERR_UNSUPPORTED, "this handle's configuration has no gated form (mppi_arm_batch)");
  hipStream_t S = nullptr;
  if (int rc = use_batch_stream(h0, &S)) return rc;
  for (int i = 0; i < n; i++)
    if (int rc = hand_over(hs[i], S)) return rc;
  QuadBatchArgs qb;
  TailLaunch tl[kMaxBatch];
  qb.n = n;
  for (int i = 0; i < n; i++)
    if (int rc = arm_handle(hs[i], 1, S, max_wait_s, false, true, qb.inst[i], tl[i])) return rc;
  for (int i = 0; i < n; i++) {
    hs[i]->arm_n = n;
    for (int q = 0; q < n; q++) hs[i]->arm_peers[q] = hs[q];
  }
  for (int i = n; i < kMaxBatch; i++) qb.inst[i] = qb.inst[0];
  hipError_t e = launch_rollout_batch(hs, n, qb, true, S);
  if (e == hipSuccess) e = launch_solve_tail_batch(tl, n, S);
  if (e != hipSuccess) {
    const int rc = fail(h0, MPPI_ERR_HIP, "armed batched launch", e);
    (void)solve_ahead_disarm(h0);
    return rc;
  }
  return MPPI_OK;
}

// the next solve's controls are finite: no explicit noise waits, and the host's nominal sequence and history are finite numbers
// (a pending solve replaces them by a weighted mean of clamped controls: not finite only where every cost already is NaN)
static bool controls_finite(const mppi_handle *h)
{
  if (h->explicit_iters > 0) return false;
  for (float u : h->U)
    if (!std::isfinite(u)) return false;
  for (float u : h->hist)
    if (!std::isfinite(u)) return false;
  return true;
}

// One launch for all instances where the quad form serves them together (every wave of every group still gets a
// SIMD of its own: the sum of the groups fits the CUs); otherwise every solve on its own handle's stream, as
// n calls of mppi_compute_control_async would do.  (mppi_compute_control_batch_async, mppi_arm_batch)
static bool batch_together(mppi_handle *const *hs, int n)
{
  const mppi_handle *h0 = hs[0];
  bool together = n >= 2 && n <= kMaxBatch;
  int waves = 0;
  for (int i = 0; i < n && together; i++) {
    const mppi_handle *h = hs[i];
    // the forms with a batched kernel (FormDesc::Batch) -- network model: the four-wavefront form, the row forms; basis-function
    // model: its three-wavefront form (in-kernel generator)
    const Form f = form_of(h);
    const FormDesc &d = form_desc(f);
    // the pair of a tick only (their batched kernels exist for two instances): the automatic m44 form of one network shape; the
    // lds44 / lds128 / glb44 form (by name only: forced on every handle) of one WHOLE layer list -- one layer list and one image size
    // serve the launch
    // (glb44: and one cap on the resident quads -- one dynamic-LDS size)
    // (... or the pair of the basis-function model's bf_row form, by name only: forced on both handles)
    const bool wide = d.batch.pair_only && !h->basis;
    bool same_list = h->net.n_layers == h0->net.n_layers;
    for (int l = 0; l < h->net.n_layers && same_list; l++) same_list = h->net.layers[l] == h0->net.layers[l];
    const bool form_ok = d.batch.launch != nullptr && (!d.batch.pair_only || n == 2) && f == form_of(h0) && h->basis == h0->basis &&
                         h->hidden == h0->hidden && h->n_hidden == h0->n_hidden && (!d.batch.same_list || same_list) &&
                         (!d.cap || h->*d.cap == h0->*d.cap);
    // one kernel instance serves the whole batch: the instances must agree on what it is specialised for (affine / projective
    // costmap transform, control cost or none) -- a superset kernel would compute 0 * x where the single solve computes
    // nothing, which differs for a non-finite x; such a pair is solved one by one.
    // The m44 / lds44 / lds128 pair may differ in the control cost: the term of an instance without one is coeff * du * (u - du) / nu^2
    // with coeff = 0 and a finite non-zero nu (fill_cost_args), exactly +0 while its controls are finite whatever the STATE is --
    // and they are: clamped draws of the in-kernel generator around a finite nominal sequence (controls_finite).  The
    // projective transform divides by a w computed from the state: that superset stays refused.
    CostArgs ci, c0;
    fill_cost_args(h, ci);
    fill_cost_args(h0, c0);
    const bool ctrl_ok = ci.need_control_cost == c0.need_control_cost || (wide && controls_finite(h) && controls_finite(h0));
    together = form_ok && ci.affine == c0.affine && ctrl_ok &&
               h->cfg.device == h0->cfg.device && h->cfg.num_iters == h0->cfg.num_iters &&
               h->K <= 4096 && !h->timing && !h->capture && !h->prefetch_valid && h->have_nn && h->have_map && h->have_cost;
    // waves of a group that need a SIMD each: quad 4, row 4 dynamics waves (its riders ride), basis functions 3 per 64 rollouts
    // (bf_row: the row form's 4 per 16)
    waves += d.batch.waves * (h->K / 64);
  }
  return together && waves <= h0->num_simds;  // every wave of every group still gets a SIMD of its own
}

// The fleet: 2..kMaxFleet handles ALL forced to "fleet16", ALL to "fleet_multi4", ALL to "fleet_bf" or ALL to "fleet_glb16" (a mixed set is
// solved handle by handle) on one device with one whole layer list (the basis-function model: one forced wave count instead; "fleet_glb16": any
// lists and caps -- they are data of its launch, FormDesc::fleet_net), one num_iters and one pair (affine
// costmap transform, control cost needed) -- one kernel instance serves the launch, and a superset kernel would not keep every
// instance's bits (batch_together) -- K <= 4096 each (the one-workgroup-per-row tail), no stage timing, capture or prefetched
// draws, every handle ready.  Such a set shares its launches: per iteration one generator, one rollout and one tail launch on
// the device's batch stream.  Anything else about the instances may differ.
static bool fleet_together(mppi_handle *const *hs, int n)
{
  if (n < 2 || n > kMaxFleet) return false;
  const mppi_handle *h0 = hs[0];
  CostArgs c0;
  fill_cost_args(h0, c0);
  for (int i = 0; i < n; i++) {
    const mppi_handle *h = hs[i];
    if (h->basis != h0->basis || !form_desc(h0->forced).fleet || h->forced != h0->forced || h->fleet_one == nullptr || h->cfg.device != h0->cfg.device || h->cfg.num_iters != h0->cfg.num_iters) return false;
    if (h->basis) {  // "fleet_bf": one wave count for the launch, forced on all or on none
      if (h->fleet_bf_waves != h0->fleet_bf_waves) return false;
    } else if (!form_desc(h0->forced).fleet_net) {
      if (h->net.n_layers != h0->net.n_layers) return false;
      for (int l = 0; l < h->net.n_layers; l++)
        if (h->net.layers[l] != h0->net.layers[l]) return false;
    }
    CostArgs ci;
    fill_cost_args(h, ci);
    if (ci.affine != c0.affine || ci.need_control_cost != c0.need_control_cost) return false;
    if (h->K > 4096 || h->K % 64 != 0 || h->timing || h->capture || h->prefetch_valid || h->armed || !h->have_nn || !h->have_map || !h->have_cost) return false;
  }
  return true;
}

// A batch batch_together admits: the instances' argument blocks travel by value (QuadBatchArgs), one rollout and one tail launch
// per iteration on the device's batch stream.
static int enqueue_pair(mppi_handle *const *hs, const float *states, int n)
{
  HP_CLOCK(hp_t);
  mppi_handle *h0 = hs[0];
  hipStream_t S = nullptr;
  if (int rc = use_batch_stream(h0, &S)) return rc;
  HP(kHpStream, hp_t);  // current device + the batch stream
  if (int rc = collect(hs, n)) return rc;
  HP(kHpWait, hp_t);  // wait_pending of every handle
  if (int rc = begin_solves(hs, n, S, true)) return distrust(hs, n, rc);
  const int iters = h0->cfg.num_iters;
  for (int it = 0; it < iters; it++) {
    QuadBatchArgs qb;
    TailLaunch tl[kMaxBatch];
    qb.n = n;
    for (int i = 0; i < n; i++)
      if (int rc = solve_step(hs[i], states + (size_t)MPPI_STATE_DIM * i, it, it == iters - 1, S, Eps::Pair, qb.inst[i], tl[i], nullptr))
        return distrust(hs, n, rc);
    for (int i = n; i < kMaxBatch; i++) qb.inst[i] = qb.inst[0];
    HP(kHpArgs, hp_t);  // uploads + argument blocks
    hipError_t e = launch_rollout_batch(hs, n, qb, false, S);
    HP(kHpPairRollout, hp_t);
    if (e == hipSuccess) e = launch_solve_tail_batch(tl, n, S);
    HP(kHpPairTail, hp_t);
    if (e != hipSuccess) return distrust(hs, n, fail(h0, MPPI_ERR_HIP, "batched launch", e));
  }
  finish_solves(hs, states, n, false);
  HP_CALL(kHpDecide);
  return MPPI_OK;
}

// The batched solve of a fleet (fleet_together).  The argument blocks of an iteration -- rollout, tail, generator -- are staged in
// the device's block and sent with one copy in front of the iteration's three launches, under the block's lock.
static int enqueue_fleet(mppi_handle *const *hs, const float *states, int n)
{
  mppi_handle *h0 = hs[0];
  hipStream_t S = nullptr;
  if (int rc = use_batch_stream(h0, &S)) return rc;
  FleetBlock *fb = fleet_block(h0->cfg.device);
  if (!fb) return fail(h0, MPPI_ERR_HIP, "no argument block for the fleet");
  if (int rc = collect(hs, n)) return rc;
  std::lock_guard<std::mutex> lk(fb->mu);
  if (int rc = begin_solves(hs, n, S, true)) return distrust(hs, n, rc);
  const int iters = h0->cfg.num_iters;
  const FormDesc &fd = form_desc(h0->forced);
  TailLaunch tl[kMaxFleet];
  for (int it = 0; it < iters; it++) {
    unsigned char *host = nullptr;
    hipError_t e = arg_block_stage(fb->args, &host);
    if (e != hipSuccess) return distrust(hs, n, fail(h0, MPPI_ERR_HIP, "fleet argument block", e));
    RolloutArgs *ra = reinterpret_cast<RolloutArgs *>(host);
    NoiseFleetDesc *nd = reinterpret_cast<NoiseFleetDesc *>(host + fleet_noise_offset(n));
    if (fd.fleet_net) {  // every instance's layer list and resident blocks: the block's fourth section
      FleetGlbNet *nets = reinterpret_cast<FleetGlbNet *>(host + fleet_net_offset(n));
      for (int i = 0; i < n; i++) nets[i] = fd.fleet_net(hs[i]);
    }
    for (int i = 0; i < n; i++)
      if (int rc = solve_step(hs[i], states + (size_t)MPPI_STATE_DIM * i, it, it == iters - 1, S, Eps::Fleet, ra[i], tl[i], &nd[i]))
        return distrust(hs, n, rc);
    fill_solve_tail_fleet(host + fleet_tail_offset(n), tl, n);
    e = arg_block_send(fb->args, fleet_bytes(n, fd.fleet_net != nullptr), S);
    const unsigned char *dev = fb->args.d;
    if (e == hipSuccess) e = launch_noise_fleet(nd, reinterpret_cast<const NoiseFleetDesc *>(dev + fleet_noise_offset(n)), n, S);
    if (e == hipSuccess)
      e = fd.fleet(hs, ra, reinterpret_cast<const RolloutArgs *>(dev), reinterpret_cast<const FleetGlbNet *>(dev + fleet_net_offset(n)), n, S);
    if (e == hipSuccess) e = launch_solve_tail_fleet(tl, n, dev + fleet_tail_offset(n), S);
    if (e != hipSuccess) return distrust(hs, n, fail(h0, MPPI_ERR_HIP, "fleet launch", e));
    for (int i = 0; i < n; i++) {
      hs[i]->launch_instances = n;
      hs[i]->launch_gated = false;
    }
  }
  finish_solves(hs, states, n, false);
  return MPPI_OK;
}

// ---- closed-loop ticks of a fleet on the device (mppi_closed_loop_ticks_batch) --------------------------------------------------
// enqueue_fleet's tick with nothing collected in between: the state stays on the device (plant_fleet_kernel writes it into the
// NEXT tick's rollout argument block, whose copy is already on the stream in front of it), the tail kernel smooths the device copy
// of U with the host's bits and leaves it slid, the generator and the argument ring advance without the host.  The host only runs
// its bookkeeping ahead -- seq, gen_cur, rng_cur, in_cur, the tail's epoch and the minimum-cost tag, as solve_step moves them -- and
// is held back by nothing but the ring's events.
static FleetWork g_loop_work[64];
static std::mutex g_loop_mu[64];  // a device's g_loop_work: held for a whole run, waits included (only another closed-loop run waits for it)
constexpr int kLoopChunkTicks = 1024;  // ticks per run of the driver: bounds the log buffers, whatever n_ticks is

int closed_loop_first_bad_tick(const float *etas, const float *controls, int n_ticks, int stride)
{
  for (int t = 0; t < n_ticks; t++) {
    if (!(etas[t] >= 1.0f) || !std::isfinite(etas[t])) return t;
    for (int j = 0; j < 2 * stride; j++)
      if (!std::isfinite(controls[(size_t)2 * stride * t + j])) return t;
  }
  return -1;
}

// does the tail's slid copy serve the slide of this run (mppi_slide_control_seq's first branch), or does slide_kernel run?
static bool loop_swaps(const mppi_handle *h, int stride) { return wants_slid_copy(h) && stride == h->cfg.optimization_stride; }

// one handle's pieces of the run's log buffer, in floats from its start
struct LoopLog {
  size_t x, u, c, e, end;
};
static LoopLog loop_log(int n_ticks, int stride)
{
  LoopLog l;
  l.x = 0;
  l.u = align4((size_t)7 * (n_ticks + 1));
  l.c = l.u + align4((size_t)2 * stride * n_ticks);
  l.e = l.c + align4((size_t)n_ticks);
  l.end = l.e + align4((size_t)n_ticks);
  return l;
}

// The wait for the run's last tick: the sequence number of handle i's result block moves with every tick, and the limit of
// mppi_set_wait_timeout applies between two moves.  false: no progress for that long.
static bool wait_for_ticks(mppi_handle *const *hs, int n, hipStream_t S)
{
  for (int i = 0; i < n; i++) {
    const mppi_handle *h = hs[i];
    const volatile unsigned *word = reinterpret_cast<const volatile unsigned *>(h->h_res) + 4 * (h->T + 1) + 1;
    unsigned seen = __atomic_load_n(word, __ATOMIC_ACQUIRE);
    auto t0 = std::chrono::steady_clock::now();
    unsigned long spins = 0;
    double next_query_s = 0.01;
    while (seen != h->seq) {
      __builtin_ia32_pause();
      const unsigned cur = __atomic_load_n(word, __ATOMIC_ACQUIRE);
      if (cur != seen) {  // a tick further
        seen = cur;
        t0 = std::chrono::steady_clock::now();
        next_query_s = 0.01;
        continue;
      }
      if ((++spins & 0xFF) != 0) continue;
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (el > h->wait_timeout_s) return false;
      if (el > next_query_s) {
        next_query_s = el + 0.01;
        if (hipStreamQuery(S) == hipSuccess) break;  // drained: wait_pending says what is missing
      }
    }
  }
  return true;
}

// n_ticks <= kLoopChunkTicks ticks of a set that is fleet_together and nominal_fleet_together with one iteration, every pending
// solve collected.  The logs may be NULL as arrays or entry by entry.  substeps == 0: mppi_closed_loop_ticks_batch, the plant step in
// plant_fleet_kernel; substeps >= 1: mppi_closed_loop_sim_batch without feedback on a set that is plant_drive_together as well, the
// plant in plant_drive_fleet_kernel (`stride` periods of `substeps` steps, the rows of U clamped by the kernel itself).
static int closed_loop_fleet(mppi_handle *const *hs, float *states, int n, int n_ticks, int stride, int substeps, float *const *state_log,
                             float *const *control_log, float *const *cost_log)
{
  const bool sim = substeps > 0;
  const int per_tick = sim ? stride * substeps : stride;  // applied controls per tick
  mppi_handle *h0 = hs[0];
  hipStream_t S = nullptr;
  if (int rc = use_batch_stream(h0, &S)) return rc;
  const int dev = h0->cfg.device;
  FleetBlock *fb = fleet_block(dev);
  if (!fb) return fail(h0, MPPI_ERR_HIP, "no argument block for the fleet");
  const FormDesc &fd = form_desc(h0->forced);
  const LoopLog lg = loop_log(n_ticks, per_tick);
  const size_t arg_floats = align4(((sim ? sizeof(PlantDriveArgs) : sizeof(PlantFleetArgs)) * (size_t)n + sizeof(float) - 1) / sizeof(float));
  const size_t in_floats = arg_floats + (size_t)8 * n, out_floats = lg.end * (size_t)n;
  if (dev < 0 || dev >= 64) return fail(h0, MPPI_ERR_INVALID, "device out of range");
  // the run's buffers for the whole run; the fleet block only while the run is enqueued: batched solves, replays and DDP passes of
  // other threads on this device queue behind the run on the stream, their callers do not sit out its waits
  std::lock_guard<std::mutex> run_lk(g_loop_mu[dev]);
  std::unique_lock<std::mutex> lk(fb->mu);
  for (int i = 0; i < n; i++) {
    hs[i]->closed_loop_on_device = 1;
    hs[i]->closed_loop_ticks = 0;
  }
  FleetWork *w = &g_loop_work[dev];
  if (in_floats > w->in_cap || out_floats > w->out_cap) {
    HIPCHK(h0, hipStreamSynchronize(S));  // nothing of an earlier run is behind the buffers
    HIPCHK(h0, fleet_grow(&w->d_in, &w->h_in, &w->in_cap, in_floats));
    HIPCHK(h0, fleet_grow(&w->d_out, &w->h_out, &w->out_cap, out_floats));
  }
  if (int rc = begin_solves(hs, n, S, true)) return distrust(hs, n, rc);
  // the plant's argument blocks (sent once) and the state slots behind them
  PlantFleetArgs *pa = reinterpret_cast<PlantFleetArgs *>(w->h_in);
  const PlantFleetArgs *d_pa = reinterpret_cast<const PlantFleetArgs *>(w->d_in);
  PlantDriveArgs *da = reinterpret_cast<PlantDriveArgs *>(w->h_in);
  const PlantDriveArgs *d_da = reinterpret_cast<const PlantDriveArgs *>(w->d_in);
  for (int i = 0; i < n; i++) {
    const mppi_handle *h = hs[i];
    float *o = w->d_out + lg.end * (size_t)i;
    memcpy(w->h_in + arg_floats + (size_t)8 * i, states + (size_t)MPPI_STATE_DIM * i, sizeof(float) * kStateDim);
    w->h_in[arg_floats + (size_t)8 * i + 7] = 0.0f;
    if (sim) {
      PlantDriveArgs &a = da[i];
      a = PlantDriveArgs{};
      plant_drive_fill(h, stride, substeps, 0, a);
      a.useq_even = h->d_in;
      a.useq_odd = loop_swaps(h, stride) ? h->d_in_buf[1 - h->in_cur] : h->d_in;
      a.clamp_rows = 1;
      a.scal = h->d_scal;
      a.state_in = a.state_out = w->d_in + arg_floats + (size_t)8 * i;
      a.applied = o + lg.u;
      a.log_x = o + lg.x; a.log_c = o + lg.c; a.log_e = o + lg.e;
      continue;
    }
    PlantFleetArgs &a = pa[i];
    a = PlantFleetArgs{};
    a.wimg = image(h, Image::Trace);
    a.U_even = h->d_in;
    a.U_odd = loop_swaps(h, stride) ? h->d_in_buf[1 - h->in_cur] : h->d_in;
    a.scal = h->d_scal;
    a.state = w->d_in + arg_floats + (size_t)8 * i;
    a.log_x = o + lg.x; a.log_u = o + lg.u; a.log_c = o + lg.c; a.log_e = o + lg.e;
    a.T = h->T;
    a.negate_yaw_der = h->cfg.negate_yaw_der ? 1 : 0;
    a.stride = stride;
    a.dt = h->dt;
    for (int j = 0; j < kControlDim; j++) { a.u_lo[j] = h->u_lo[j]; a.u_hi[j] = h->u_hi[j]; }
    a.net = h->net;
  }
  // the plant step behind tick `tick`; ra: the next tick's rollout argument blocks in device memory, or nullptr
  auto launch_plant = [&](RolloutArgs *ra, int tick) -> hipError_t {
    return sim ? launch_plant_drive_fleet(da, d_da, ra, n, tick, S) : launch_plant_fleet(pa, d_pa, ra, n, tick, S);
  };
  hipError_t e = hipMemcpyAsync(w->d_in, w->h_in, sizeof(float) * in_floats, hipMemcpyHostToDevice, S);
  if (e != hipSuccess) return distrust(hs, n, fail(h0, MPPI_ERR_HIP, "closed loop: input copy", e));
  // behind plant step `tick`: the slide of every handle whose slid copy is not simply swapped in (the swap itself is the host's)
  auto slide_behind_plant = [&]() -> hipError_t {
    for (int i = 0; i < n; i++) {
      const mppi_handle *h = hs[i];
      if (loop_swaps(h, stride)) continue;
      if (hipError_t es = launch_slide(h->d_in, h->T, stride, h->cfg.init_control[0], h->cfg.init_control[1], S); es != hipSuccess) return es;
    }
    return hipSuccess;
  };
  static const float no_state[kStateDim] = {0, 0, 0, 0, 0, 0, 0};  // ticks after the first: plant_fleet_kernel writes the block's state
  TailLaunch tl[kMaxFleet];
  for (int tick = 0; tick < n_ticks; tick++) {
    unsigned char *host = nullptr;
    e = arg_block_stage(fb->args, &host);  // the run's one wait: the copy out of this slot, four ticks ago
    if (e != hipSuccess) return distrust(hs, n, fail(h0, MPPI_ERR_HIP, "fleet argument block", e));
    RolloutArgs *ra = reinterpret_cast<RolloutArgs *>(host);
    NoiseFleetDesc *nd = reinterpret_cast<NoiseFleetDesc *>(host + fleet_noise_offset(n));
    if (fd.fleet_net) {
      FleetGlbNet *nets = reinterpret_cast<FleetGlbNet *>(host + fleet_net_offset(n));
      for (int i = 0; i < n; i++) nets[i] = fd.fleet_net(hs[i]);
    }
    for (int i = 0; i < n; i++) {
      mppi_handle *h = hs[i];
      if (tick > 0) {  // begin_solves' share of a tick
        h->seq = next_seq(h);
        forget_solve_state(h);
      }
      if (int rc = solve_step(h, tick == 0 ? states + (size_t)MPPI_STATE_DIM * i : no_state, 0, true, S, Eps::Fleet, ra[i], tl[i], &nd[i]))
        return distrust(hs, n, rc);
    }
    fill_solve_tail_fleet(host + fleet_tail_offset(n), tl, n);
    e = arg_block_send(fb->args, fleet_bytes(n, fd.fleet_net != nullptr), S);
    unsigned char *dev_blk = fb->args.d;
    // the plant step of the tick before, BEHIND this tick's argument copy: its state lands in the block the rollout reads
    if (e == hipSuccess && tick > 0) e = launch_plant(reinterpret_cast<RolloutArgs *>(dev_blk), tick - 1);
    if (e == hipSuccess && tick > 0) e = slide_behind_plant();
    if (e == hipSuccess) e = launch_noise_fleet(nd, reinterpret_cast<const NoiseFleetDesc *>(dev_blk + fleet_noise_offset(n)), n, S);
    if (e == hipSuccess)
      e = fd.fleet(hs, ra, reinterpret_cast<const RolloutArgs *>(dev_blk), reinterpret_cast<const FleetGlbNet *>(dev_blk + fleet_net_offset(n)), n, S);
    if (e == hipSuccess) e = launch_solve_tail_fleet(tl, n, dev_blk + fleet_tail_offset(n), S);
    if (e != hipSuccess) return distrust(hs, n, fail(h0, MPPI_ERR_HIP, "closed loop: fleet launch", e));
    for (int i = 0; i < n; i++) {
      mppi_handle *h = hs[i];
      h->launch_instances = n;
      h->launch_gated = false;
      // mppi_slide_control_seq's device half, the host's side of it: the slid copy the tail leaves is the next tick's sequence
      if (loop_swaps(h, stride)) {
        h->in_cur = 1 - h->in_cur;
        h->d_in = h->d_in_buf[h->in_cur];
      }
    }
  }
  e = launch_plant(nullptr, n_ticks - 1);
  if (e == hipSuccess) e = slide_behind_plant();
  if (e == hipSuccess) e = hipMemcpyAsync(w->h_out, w->d_out, sizeof(float) * out_floats, hipMemcpyDeviceToHost, S);
  for (int i = 0; i < n && e == hipSuccess; i++)  // the smoothed and slid [U | hist]: what the host's copies become
    e = hipMemcpyAsync(hs[i]->h_in, hs[i]->d_in, sizeof(float) * (2 * (size_t)hs[i]->T + 4), hipMemcpyDeviceToHost, S);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(S);
    return distrust(hs, n, fail(h0, MPPI_ERR_HIP, "closed loop: plant step / result copy", e));
  }
  for (int i = 0; i < n; i++) {  // finish_solves' share: the last tick is a pending solve like any other
    hs[i]->explicit_iters = 0;
    hs[i]->pending = true;
    hs[i]->pending_timed = false;
  }
  lk.unlock();  // everything is enqueued: the waits below hold only the run's own buffers
  if (!wait_for_ticks(hs, n, S)) {
    // as a solve whose wait ran out of time: nothing waits for the run again until its device work has drained
    for (int i = 0; i < n; i++) {
      mppi_handle *h = hs[i];
      h->pending = false;
      h->u_dirty = true;
      h->slid_valid = false;
      h->timed_out = true;
      h->no_result = true;
      fail(h, MPPI_ERR_HIP, "closed loop: timed out waiting for a tick");
    }
    return MPPI_ERR_HIP;
  }
  int rc = MPPI_OK;
  for (int i = 0; i < n; i++) {  // (smooths the host's U from the result block with the OLD history: replaced below)
    const int r = wait_pending(hs[i]);
    if (r && !rc) rc = r;
  }
  e = hipStreamSynchronize(S);
  if (e != hipSuccess) return distrust(hs, n, fail(h0, MPPI_ERR_HIP, "closed loop: synchronise", e));
  // the host's check behind the run: the ticks ran on after a bad one
  int bad_tick = -1, bad_handle = -1;
  for (int i = 0; i < n; i++) {
    const float *o = w->h_out + lg.end * (size_t)i;
    const int t = closed_loop_first_bad_tick(o + lg.e, o + lg.u, n_ticks, per_tick);
    if (t >= 0 && (bad_tick < 0 || t < bad_tick)) {
      bad_tick = t;
      bad_handle = i;
    }
  }
  const int good_ticks = bad_tick >= 0 ? bad_tick : (rc ? 0 : n_ticks);
  for (int i = 0; i < n; i++) {
    const float *o = w->h_out + lg.end * (size_t)i;
    if (state_log && state_log[i]) {
      memcpy(state_log[i], states + (size_t)MPPI_STATE_DIM * i, sizeof(float) * kStateDim);
      memcpy(state_log[i] + 7, o + lg.x + 7, sizeof(float) * 7 * (size_t)good_ticks);
    }
    if (control_log && control_log[i]) memcpy(control_log[i], o + lg.u, sizeof(float) * 2 * (size_t)per_tick * good_ticks);
    if (cost_log && cost_log[i]) memcpy(cost_log[i], o + lg.c, sizeof(float) * (size_t)good_ticks);
    hs[i]->closed_loop_on_device = 1;
    hs[i]->closed_loop_ticks = good_ticks;
  }
  if (bad_tick >= 0 || rc) {  // (the caller puts the host's U / history and the states back)
    for (int i = 0; i < n; i++) hs[i]->no_result = true;
    if (bad_tick >= 0) {
      char msg[160];
      snprintf(msg, sizeof(msg), "closed loop: tick %d of handle %d produced a non-finite normaliser or controls", bad_tick, bad_handle);
      fail(hs[bad_handle], MPPI_ERR_HIP, msg);
      rc = fail(h0, MPPI_ERR_HIP, msg);
    }
    return distrust(hs, n, rc);
  }
  for (int i = 0; i < n; i++) {
    mppi_handle *h = hs[i];
    const float *o = w->h_out + lg.end * (size_t)i;
    memcpy(h->U.data(), h->h_in, sizeof(float) * 2 * (size_t)h->T);
    memcpy(h->hist.data(), h->h_in + 2 * h->T, sizeof(float) * 4);
    h->u_dirty = false;
    h->slid_valid = false;  // as behind mppi_slide_control_seq
    // the last solve's state: the log's row n_ticks - 1 -- row 0 is the host's (the kernel writes rows 1 .. n_ticks)
    note_solve_state(h, n_ticks == 1 ? states + (size_t)MPPI_STATE_DIM * i : o + lg.x + (size_t)7 * (n_ticks - 1), true);
    memcpy(states + (size_t)MPPI_STATE_DIM * i, o + lg.x + (size_t)7 * n_ticks, sizeof(float) * kStateDim);
  }
  return MPPI_OK;
}

// the loop of public calls itself: the reference of the device path, and what every other set runs
static int closed_loop_reference(mppi_handle *const *hs, float *states, int n, int n_ticks, int stride, float *const *state_log,
                                 float *const *control_log, float *const *cost_log)
{
  std::vector<std::vector<float>> xs(n), us(n);
  std::vector<float *> xp(n), up(n);
  for (int i = 0; i < n; i++) {
    xs[i].resize((size_t)hs[i]->T * kStateDim);
    us[i].resize((size_t)hs[i]->T * kControlDim);
    xp[i] = xs[i].data();
    up[i] = us[i].data();
    hs[i]->closed_loop_on_device = 0;
    hs[i]->closed_loop_ticks = 0;
  }
  for (int tick = 0; tick < n_ticks; tick++) {
    int rc = mppi_compute_control_batch(hs, states, n);
    if (rc == MPPI_OK) rc = mppi_nominal_traj_batch(hs, states, xp.data(), up.data(), n);
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
      float *s = states + (size_t)MPPI_STATE_DIM * i;
      if (state_log && state_log[i]) memcpy(state_log[i] + (size_t)7 * tick, s, sizeof(float) * kStateDim);
      if (control_log && control_log[i]) memcpy(control_log[i] + (size_t)2 * stride * tick, up[i], sizeof(float) * 2 * (size_t)stride);
      if (cost_log && cost_log[i]) cost_log[i][tick] = hs[i]->traj_cost;
      memcpy(s, xp[i] + (size_t)7 * stride, sizeof(float) * kStateDim);
      if (state_log && state_log[i]) memcpy(state_log[i] + (size_t)7 * (tick + 1), s, sizeof(float) * kStateDim);
      rc = mppi_slide_control_seq(hs[i], stride);
      if (rc) return rc;
      hs[i]->closed_loop_ticks = tick + 1;
    }
  }
  return MPPI_OK;
}

// mppi_closed_loop_sim_batch's loop of public calls: its definition, and what every set without a device path runs
static int closed_loop_sim_reference(mppi_handle *const *hs, float *states, int n, int n_ticks, int stride, int substeps, int feedback,
                                     float *const *state_log, float *const *control_log, float *const *cost_log)
{
  const size_t per_tick = (size_t)stride * substeps;
  std::vector<std::vector<float>> xs(n), us(n), ap(n);
  std::vector<float *> xp(n), up(n), app(n);
  std::vector<float> s_next((size_t)MPPI_STATE_DIM * n);
  for (int i = 0; i < n; i++) {
    xs[i].resize((size_t)hs[i]->T * kStateDim);
    us[i].resize((size_t)hs[i]->T * kControlDim);
    ap[i].resize(2 * per_tick);
    xp[i] = xs[i].data();
    up[i] = us[i].data();
    app[i] = ap[i].data();
    hs[i]->closed_loop_on_device = 0;
    hs[i]->closed_loop_ticks = 0;
  }
  for (int tick = 0; tick < n_ticks; tick++) {
    int rc = mppi_compute_control_batch(hs, states, n);
    if (rc == MPPI_OK)
      rc = feedback ? mppi_nominal_and_gains_batch(hs, states, xp.data(), up.data(), n) : mppi_nominal_traj_batch(hs, states, xp.data(), up.data(), n);
    if (rc == MPPI_OK) rc = mppi_plant_drive_batch(hs, states, xp.data(), up.data(), n, stride, substeps, feedback, s_next.data(), app.data());
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
      float *s = states + (size_t)MPPI_STATE_DIM * i;
      if (state_log && state_log[i]) memcpy(state_log[i] + (size_t)7 * tick, s, sizeof(float) * kStateDim);
      if (control_log && control_log[i]) memcpy(control_log[i] + 2 * per_tick * tick, app[i], sizeof(float) * 2 * per_tick);
      if (cost_log && cost_log[i]) cost_log[i][tick] = hs[i]->traj_cost;
      memcpy(s, s_next.data() + (size_t)MPPI_STATE_DIM * i, sizeof(float) * kStateDim);
      if (state_log && state_log[i]) memcpy(state_log[i] + (size_t)7 * (tick + 1), s, sizeof(float) * kStateDim);
      rc = mppi_slide_control_seq(hs[i], stride);
      if (rc) return rc;
      hs[i]->closed_loop_ticks = tick + 1;
    }
  }
  return MPPI_OK;
}

static bool armed_as_batch(mppi_handle *const *hs, int n)
{
  for (int i = 0; i < n; i++) {
    if (!hs[i]->armed || hs[i]->arm_n != n) return false;
    for (int q = 0; q < n; q++)
      if (hs[i]->arm_peers[q] != hs[q]) return false;
  }
  return true;
}

}  // namespace mppi_abi

extern "C" {

int mppi_compute_control_async(mppi_handle *h, const float state[MPPI_STATE_DIM])
{
  if (!h) return MPPI_ERR_INVALID;
  HIPCHK(h, ensure_device(h->cfg.device));
  return enqueue_solve(h, state);
}

int mppi_synchronize(mppi_handle *h)
{
  if (!h) return MPPI_ERR_INVALID;
  return wait_pending(h);
}

int mppi_compute_control(mppi_handle *h, const float state[MPPI_STATE_DIM])
{
  int rc = mppi_compute_control_async(h, state);
  if (rc) return rc;
  return mppi_synchronize(h);
}

int mppi_compute_control_batch_async(mppi_handle *const *hs, const float *states, int n)
{
  if (!hs || !states || n < 1) return MPPI_ERR_INVALID;
  HP_CLOCK(hp_t);
  for (int i = 0; i < n; i++) {
    if (!hs[i]) return MPPI_ERR_INVALID;
    for (int q = 0; q < i; q++)
      if (hs[q] == hs[i]) return fail(hs[i], MPPI_ERR_INVALID, "the same handle twice in one batch");
  }
  // the host-side halves of this tick (nominal replays, DDP passes) are a solve's length away: the helper thread wakes now
  if (n == 2 && g_host_threads.load(std::memory_order_relaxed) >= 2) host_helper_arm();
  // armed together (mppi_arm_batch) with exactly these handles in this order: the gates open.  Any other batch calls the
  // armed solves of its handles off first.
  if (armed_as_batch(hs, n)) {
    int rc = MPPI_OK;
    bool usable = true;
    for (int i = 0; i < n; i++) {
      mppi_handle *h = hs[i];
      if (rc == MPPI_OK) rc = check_ready(h);
      if (rc == MPPI_OK) rc = recover_timed_out(h);
      if (rc == MPPI_OK) rc = wait_pending(h);
      usable = usable && arm_usable(h);
    }
    if (rc == MPPI_OK && usable) {
      for (int i = 0; i < n; i++) {
        const int orc = open_armed(hs[i], states + (size_t)MPPI_STATE_DIM * i);
        if (orc && !rc) rc = orc;
      }
      return rc;
    }
    const int drc = solve_ahead_disarm(hs[0]);
    if (rc) return rc;
    if (drc) return drc;
  }
  const bool together = batch_together(hs, n);
  for (int i = 0; i < n; i++) {  // an armed solve of another batch; one armed alone where this batch is one launch
    if (hs[i]->armed && (hs[i]->arm_n > 0 || together)) {
      const int drc = solve_ahead_disarm(hs[i]);
      if (drc) return drc;
    }
  }
  mppi_handle *h0 = hs[0];
  if (!together && fleet_together(hs, n)) return enqueue_fleet(hs, states, n);  // the fleet forms: 2..64 handles, three launches
  if (!together && n >= 2) {
    // a set of handles of one fleet form with one that is not ready: its error before any of the others has moved
    bool all_fleet = form_desc(h0->forced).fleet != nullptr;
    for (int i = 0; i < n; i++) all_fleet = all_fleet && hs[i]->forced == h0->forced;
    for (int i = 0; i < n && all_fleet; i++)
      if (const int rc = check_ready(hs[i])) return rc;
  }
  if (!together) {
    for (int i = 0; i < n; i++) {
      const int rc = mppi_compute_control_async(hs[i], states + (size_t)MPPI_STATE_DIM * i);
      if (rc) return rc;
    }
    return MPPI_OK;
  }
  HP(kHpDecide, hp_t);  // the decision: one launch for all?
  return enqueue_pair(hs, states, n);
}

int mppi_compute_control_batch(mppi_handle *const *hs, const float *states, int n)
{
  int rc = mppi_compute_control_batch_async(hs, states, n);
  for (int i = 0; i < n && rc == MPPI_OK; i++) rc = mppi_synchronize(hs[i]);
  return rc;
}

int mppi_control_ticks_batch(mppi_handle *const *hs, const float *states, int n, int n_ticks, int stride)
{
  if (!hs || !states || n < 1 || n_ticks < 0 || stride < 0) return MPPI_ERR_INVALID;
  for (int t = 0; t < n_ticks; t++) {
    int rc = mppi_compute_control_batch(hs, states, n);
    if (rc) return rc;
    for (int i = 0; i < n && stride > 0; i++) {
      rc = mppi_slide_control_seq(hs[i], stride);
      if (rc) return rc;
    }
  }
  return MPPI_OK;
}

// mppi_closed_loop_ticks_batch (substeps == 0: the plant is the controller's own model, one step per period) and
// mppi_closed_loop_sim_batch (substeps >= 1: the handle's plant under the drive law)
static int closed_loop_entry(mppi_handle *const *hs, float *states, int n, int n_ticks, int stride, int substeps, int feedback,
                             float *const *state_log, float *const *control_log, float *const *cost_log)
{
  const bool sim = substeps > 0;
  const size_t per_tick = sim ? (size_t)stride * substeps : (size_t)stride;
  // mppi_nominal_traj_batch's order: every argument, then every handle's readiness, then pending and armed solves; only then a move
  if (!hs || !states || n < 1 || n_ticks < 1) return MPPI_ERR_INVALID;
  for (int i = 0; i < n; i++) {
    if (!hs[i]) return MPPI_ERR_INVALID;
    for (int q = 0; q < i; q++)
      if (hs[q] == hs[i]) return fail(hs[i], MPPI_ERR_INVALID, "the same handle twice in one batch");
  }
  for (int i = 0; i < n; i++)
    if (stride < 1 || stride >= hs[i]->T) return fail(hs[i], MPPI_ERR_INVALID, "closed loop: stride must be in [1, T)");
  for (int i = 0; i < n; i++)
    if (const int rc = check_ready(hs[i])) return rc;
  if (const int rc = collect(hs, n)) return rc;
  for (int i = 0; i < n; i++) DISARM(hs[i]);
  bool on_device = fleet_together(hs, n) && nominal_fleet_together(hs, n) && hs[0]->cfg.num_iters == 1;
  for (int i = 0; i < n && on_device; i++) on_device = hs[i]->explicit_iters == 0;
  // MPPI_CLOSED_LOOP_DEVICE=0 (tools only, read at every call): the loop of public calls for every set -- tools/fleet_time.py
  // --closed-loop times the two against each other in one process
  if (const char *sw = getenv("MPPI_CLOSED_LOOP_DEVICE"); sw && atoi(sw) == 0) on_device = false;
  // the plant of its own: without feedback, where the drive shares a launch too; with feedback the loop of public calls
  if (sim) on_device = on_device && !feedback && plant_drive_together(hs, n);
  if (!on_device && sim) return closed_loop_sim_reference(hs, states, n, n_ticks, stride, substeps, feedback, state_log, control_log, cost_log);
  if (!on_device) return closed_loop_reference(hs, states, n, n_ticks, stride, state_log, control_log, cost_log);
  std::vector<float *> xl(n, nullptr), ul(n, nullptr), cl(n, nullptr);
  // what the host holds before the call: all of it comes back where a tick turns out bad, in whichever piece of a long run
  std::vector<std::vector<float>> keep_U(n), keep_hist(n);
  for (int i = 0; i < n; i++) {
    keep_U[i] = hs[i]->U;
    keep_hist[i] = hs[i]->hist;
  }
  const std::vector<float> keep_states(states, states + (size_t)MPPI_STATE_DIM * n);
  for (int at = 0; at < n_ticks; at += kLoopChunkTicks) {  // (a long run: its logs come back chunk by chunk)
    for (int i = 0; i < n; i++) {
      xl[i] = (state_log && state_log[i]) ? state_log[i] + (size_t)7 * at : nullptr;
      ul[i] = (control_log && control_log[i]) ? control_log[i] + 2 * per_tick * at : nullptr;
      cl[i] = (cost_log && cost_log[i]) ? cost_log[i] + at : nullptr;
    }
    const int rc = closed_loop_fleet(hs, states, n, std::min(kLoopChunkTicks, n_ticks - at), stride, substeps, xl.data(), ul.data(), cl.data());
    for (int i = 0; i < n; i++) hs[i]->closed_loop_ticks += at;
    if (rc) {  // the host's copies go back, and the next solve uploads them (an earlier piece has moved the device copy)
      for (int i = 0; i < n; i++) {
        hs[i]->U = keep_U[i];
        hs[i]->hist = keep_hist[i];
        hs[i]->u_dirty = true;
        hs[i]->slid_valid = false;
      }
      memcpy(states, keep_states.data(), sizeof(float) * keep_states.size());
      return rc;
    }
  }
  return MPPI_OK;
}

int mppi_closed_loop_ticks_batch(mppi_handle *const *hs, float *states, int n, int n_ticks, int stride, float *const *state_log,
                                 float *const *control_log, float *const *cost_log)
{
  return closed_loop_entry(hs, states, n, n_ticks, stride, 0, 0, state_log, control_log, cost_log);
}

int mppi_closed_loop_sim_batch(mppi_handle *const *hs, float *states, int n, int n_ticks, int stride, int substeps, int feedback,
                               float *const *state_log, float *const *control_log, float *const *cost_log)
{
  if (substeps < 1 || substeps > kPlantDriveMaxSubsteps) return MPPI_ERR_INVALID;
  return closed_loop_entry(hs, states, n, n_ticks, stride, substeps, feedback, state_log, control_log, cost_log);
}

int mppi_debug_closed_loop_info(const mppi_handle *h, int *on_device, int *ticks)
{
  if (!h || !on_device || !ticks) return MPPI_ERR_INVALID;
  *on_device = h->closed_loop_on_device;
  *ticks = h->closed_loop_ticks;
  return MPPI_OK;
}

int mppi_debug_closed_loop_check(const float *etas, const float *controls, int n_ticks, int stride, int *bad_tick)
{
  if (!etas || !controls || !bad_tick || n_ticks < 1 || stride < 1) return MPPI_ERR_INVALID;
  *bad_tick = closed_loop_first_bad_tick(etas, controls, n_ticks, stride);
  return MPPI_OK;
}

int mppi_control_ticks(mppi_handle *h, const float state[MPPI_STATE_DIM], int n_ticks, int stride)
{
  if (!h || n_ticks < 0 || stride < 0) return MPPI_ERR_INVALID;
  DISARM(h);
  if (state && h->chain && n_ticks >= 2 && stride == h->cfg.optimization_stride && arm_kind(h)) {
    // chained: tick i+1 is armed behind solve i (kernel deadline 100 ms), its gate opened once the host holds result i, slid
    HIPCHK(h, ensure_device(h->cfg.device));
    int rc = enqueue_solve(h, state);
    for (int i = 0; i < n_ticks && rc == MPPI_OK; i++) {
      const bool ahead = i + 1 < n_ticks;
      if (ahead) rc = arm_one(h, 0.1, i + 2 < n_ticks, false);
      if (rc == MPPI_OK) rc = wait_pending(h);
      if (rc == MPPI_OK) rc = mppi_slide_control_seq(h, stride);
      if (rc == MPPI_OK && ahead) rc = enqueue_solve(h, state);
    }
    if (rc) (void)solve_ahead_disarm(h);  // never blocks
    return rc;
  }
  for (int i = 0; i < n_ticks; i++) {
    int rc = mppi_compute_control(h, state);
    if (rc) return rc;
    if (stride > 0) {
      rc = mppi_slide_control_seq(h, stride);
      if (rc) return rc;
    }
  }
  return MPPI_OK;
}

int mppi_get_results(mppi_handle *h, float *U, float *traj_cost, float *costs, float *weights)
{
  if (!h) return MPPI_ERR_INVALID;
  int rc = mppi_synchronize(h);
  if (rc) return rc;
  if (h->no_result) return fail(h, MPPI_ERR_HIP, "the last solve timed out: no result");
  if (U) memcpy(U, h->U.data(), sizeof(float) * 2 * (size_t)h->T);
  if (traj_cost) *traj_cost = h->traj_cost;
  if ((costs || weights) && h->armed) {
    // the armed solve writes the other pair of vectors: these are the last result's once the stream has passed the point in
    // front of the armed solve (the blocking copies of the null stream do not wait for the handle's non-blocking streams)
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipEventSynchronize(h->ev_arm));
  } else if (costs || weights) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    OWN(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  if (costs) HIPCHK(h, hipMemcpy(costs, h->d_costs, sizeof(float) * h->K, hipMemcpyDeviceToHost));
  if (weights) HIPCHK(h, hipMemcpy(weights, h->d_w, sizeof(float) * h->K, hipMemcpyDeviceToHost));
  return MPPI_OK;
}

int mppi_get_applied_controls(mppi_handle *h, float *V, size_t n)
{
  if (!h || !V) return MPPI_ERR_INVALID;
  const size_t slot = (size_t)h->K * h->T * 2;
  if (n != slot) return fail(h, MPPI_ERR_INVALID, "n != K*T*2");
  int rc = mppi_synchronize(h);
  if (rc) return rc;
  if (h->no_result) return fail(h, MPPI_ERR_HIP, "the last solve timed out: no result");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (h->armed) {
    // the armed solve leaves its applied controls elsewhere: the last solve's are read on the generator stream, behind the
    // point in front of the armed solve, not behind the armed kernels
    HIPCHK(h, hipStreamWaitEvent(h->gstream, h->ev_arm, 0));
    HIPCHK(h, launch_tk_to_kt(h->v_buf, h->d_stage, h->K, h->T, h->gstream));
    HIPCHK(h, hipMemcpyAsync(V, h->d_stage, slot * sizeof(float), hipMemcpyDeviceToHost, h->gstream));
    HIPCHK(h, hipStreamSynchronize(h->gstream));
    return MPPI_OK;
  }
  OWN(h);
  HIPCHK(h, launch_tk_to_kt(h->v_buf, h->d_stage, h->K, h->T, h->stream));
  HIPCHK(h, hipMemcpyAsync(V, h->d_stage, slot * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MPPI_OK;
}

int mppi_rollout_only(mppi_handle *h, const float state[MPPI_STATE_DIM], float *costs)
{
  int rc = check_ready(h);
  if (rc) return rc;
  if (!state || !costs) return fail(h, MPPI_ERR_INVALID, "NULL argument");
  DISARM(h);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  rc = recover_timed_out(h);
  if (rc) return rc;
  rc = mppi_synchronize(h);
  if (rc) return rc;
  OWN(h);
  rc = upload_controls_if_dirty(h, h->stream);
  if (rc) return rc;
  float *noise = nullptr;  // (explicit noise: its first iteration)
  bool in_kernel = false;
  rc = eps_source(h, Eps::Single, 0, &noise, &in_kernel, nullptr);
  if (rc) return rc;
  h->explicit_iters = 0;
  forget_solve_state(h);
  RolloutArgs a;
  fill_rollout_args(h, state, noise, a);
  if (in_kernel) use_inline_noise(h, a);
  rc = launch_rollout(h, a);
  if (rc) return rc;
  note_solve_state(h, state, false);
  HIPCHK(h, hipMemcpyAsync(costs, h->d_costs, sizeof(float) * h->K, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MPPI_OK;
}

/* Debug/test entries (not part of the drop-in surface): what every iteration of a multi-iteration solve left, so that
 * a test can hold iteration i against the oracle started from the SAME U (mppi_controller.cu:609-667: the loop re-uses
 * U_ without smoothing in between).  Capturing adds two small device copies per iteration and keeps the handle out of
 * batched launches. */
int mppi_debug_capture_iterations(mppi_handle *h, int on)
{
  if (!h) return MPPI_ERR_INVALID;
  DISARM(h);
  int rc = mppi_synchronize(h);
  if (rc) return rc;
  if (on && !h->d_cap) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMalloc(&h->d_cap, sizeof(float) * (size_t)h->cfg.num_iters * (2 * (size_t)h->T + h->K)));
  }
  h->capture = on != 0;
  h->cap_valid = false;
  return MPPI_OK;
}

int mppi_debug_get_iterations(mppi_handle *h, float *U_raw, float *costs, float *V)
{
  if (!h) return MPPI_ERR_INVALID;
  int rc = mppi_synchronize(h);
  if (rc) return rc;
  if (!h->cap_valid) return fail(h, MPPI_ERR_STATE, "no captured solve (mppi_debug_capture_iterations, then a solve on this handle alone)");
  if (V && !h->cap_explicit) return fail(h, MPPI_ERR_STATE, "applied controls of every iteration exist for explicit-noise solves only");
  const int iters = h->cfg.num_iters, T = h->T, K = h->K;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  OWN(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const size_t rec = 2 * (size_t)T + K;
  std::vector<float> buf((size_t)iters * rec);
  HIPCHK(h, hipMemcpy(buf.data(), h->d_cap, sizeof(float) * buf.size(), hipMemcpyDeviceToHost));
  for (int it = 0; it < iters; it++) {
    if (U_raw) {
      float *u = U_raw + (size_t)it * 2 * T;
      if (it < iters - 1) memcpy(u, buf.data() + (size_t)it * rec, sizeof(float) * 2 * (size_t)T);
      else for (int t = 0; t < T; t++) { u[2 * t] = h->h_res[4 * t]; u[2 * t + 1] = h->h_res[4 * t + 2]; }  // rows [u0, seq, u1, seq]
    }
    if (costs) memcpy(costs + (size_t)it * K, buf.data() + (size_t)it * rec + 2 * (size_t)T, sizeof(float) * (size_t)K);
    if (V) {
      const size_t slot = (size_t)K * T * 2;
      HIPCHK(h, launch_tk_to_kt(h->d_noise + (size_t)it * slot, h->d_stage, K, T, h->stream));
      HIPCHK(h, hipMemcpyAsync(V + (size_t)it * slot, h->d_stage, slot * sizeof(float), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
  }
  return MPPI_OK;
}

/* How long a blocking call polls for a solve's result block before it reports MPPI_ERR_HIP (default 30 s).  The clock is
 * read every 256 polls: the limit holds to microseconds.  After a timeout the handle is "timed out": the host copies of U and
 * the control history are what the next solve starts from, no call waits for the lost solve again (each returns MPPI_ERR_HIP at
 * once while its device work is still running, one hipStreamQuery per call) and the handle works again once that work has
 * drained.  mppi_destroy synchronises the handle's streams and may block for as long as that work runs. */
/* Solve-ahead (csrc/abi_solve.hip: mppi_arm). */
int mppi_arm(mppi_handle *h, double max_wait_s)
{
  if (!h || !(max_wait_s > 0.0 && max_wait_s <= 0.1)) return MPPI_ERR_INVALID;
  if (h->armed && h->arm_n == 0) return MPPI_OK;  // already armed
  DISARM(h);  // (armed as part of a batch)
  HIPCHK(h, ensure_device(h->cfg.device));
  return arm_one(h, max_wait_s, false, true);
}

int mppi_arm_batch(mppi_handle *const *hs, int n, double max_wait_s)
{
  if (!hs || n < 1 || n > 64 || !(max_wait_s > 0.0 && max_wait_s <= 0.1)) return MPPI_ERR_INVALID;
  for (int i = 0; i < n; i++) {
    if (!hs[i]) return MPPI_ERR_INVALID;
    for (int q = 0; q < i; q++)
      if (hs[q] == hs[i]) return fail(hs[i], MPPI_ERR_INVALID, "the same handle twice in one batch");
  }
  if (n >= 2 && armed_as_batch(hs, n)) return MPPI_OK;
  for (int i = 0; i < n; i++)
    if (hs[i]->armed && (hs[i]->arm_n > 0 || n >= 2)) DISARM(hs[i]);
  if (n >= 2) {
    for (int i = 0; i < n; i++) {  // the batch's own checks first (what batch_together reads)
      int rc = check_ready(hs[i]);
      if (rc) return rc;
    }
    if (batch_together(hs, n)) return arm_together(hs, n, max_wait_s);
  }
  // each handle on its own, where it can be: MPPI_ERR_UNSUPPORTED if one could not be (the others stay armed)
  int out = MPPI_OK;
  for (int i = 0; i < n; i++) {
    const int rc = mppi_arm(hs[i], max_wait_s);
    if (rc == MPPI_ERR_UNSUPPORTED) out = rc;
    else if (rc) return rc;
  }
  return out;
}

int mppi_disarm(mppi_handle *h)
{
  if (!h) return MPPI_ERR_INVALID;
  return solve_ahead_disarm(h);
}

int mppi_is_armed(const mppi_handle *h)
{
  return (h && h->armed) ? 1 : 0;
}

int mppi_debug_launch_info(mppi_handle *h, int *instances, int *gated)
{
  if (!h || !instances || !gated) return MPPI_ERR_INVALID;
  *instances = h->launch_instances;
  *gated = h->launch_gated ? 1 : 0;
  return MPPI_OK;
}

int mppi_set_wait_timeout(mppi_handle *h, double seconds)
{
  if (!h || !(seconds > 0.0)) return MPPI_ERR_INVALID;
  h->wait_timeout_s = seconds;
  return MPPI_OK;
}

}  // extern "C"
