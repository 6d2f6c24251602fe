// abi_host.hip -- the host-side halves of a control tick: nominal trajectory replays (mppi_controller.cu:501-519), DDP
// feedback gains (:402-445), and the helper thread that takes one of a pair (mppi_set_host_threads); the DDP passes of a whole
// fleet in one launch of ddp_fleet_kernel (mppi_compute_feedback_gains_batch) and its nominal replays in one launch of
// nominal_fleet_kernel (mppi_nominal_traj_batch), or both in one launch of nominal_gains_fleet_kernel
// (mppi_nominal_and_gains_batch): the entries here that compute on the device.  A plant of its own per handle
// (mppi_set_plant_model) and its drive law -- the host text plant_drive_host beside the nominal replay, and the plants of a whole
// fleet in one launch of plant_drive_fleet_kernel (mppi_plant_drive_batch).
#include "abi_internal.hpp"

#include <stdexcept>

using namespace mppi;
using namespace mppi_abi;

namespace mppi_abi {

// One helper thread for the host-side halves of a control tick that come in pairs (the two controllers' nominal replays,
// their two DDP passes: run_control_loop.cuh:218-225 -- independent work on two handles): the caller's thread does one, the
// helper the other.  Off unless mppi_set_host_threads(2) was called.  The helper sleeps on a condition variable; arm() wakes it
// (mppi_compute_control_batch_async does, a solve's length before the replays are due) and it then polls for work for 1 ms
// after the last job, so that the hand-over costs a cache line, not a futex wake.
class HostHelper {
 public:
  ~HostHelper()
  {
    if (!th_.joinable()) return;
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_ = true;
      wake_ = true;
    }
    cv_.notify_one();
    th_.join();
  }
  void arm()
  {
    std::call_once(started_, [this] { th_ = std::thread([this] { loop(); }); });
    if (spinning_.load()) return;  // (seq_cst, with the stores in run_pair / loop: a job is never posted to a helper going to sleep unseen)
    {
      std::lock_guard<std::mutex> lk(mu_);
      wake_ = true;
    }
    cv_.notify_one();
  }
  // runs `other` on the helper and `mine` on the caller's thread; returns when both are done.  One pair at a time: a second
  // caller (another control loop of the process) runs both halves itself.
  void run_pair(const std::function<void()> &other, const std::function<void()> &mine)
  {
    std::unique_lock<std::mutex> busy(pair_mu_, std::try_to_lock);
    if (!busy.owns_lock()) {
      mine();
      other();
      return;
    }
    job_ = &other;
    failed_.store(false);
    done_.store(false);
    posted_.store(true);
    arm();
    // the caller leaves only after the helper is through with `other` (which refers to the caller's frame), whatever
    // `mine` does: an exception of `mine` is rethrown after the wait, one of `other` (caught on the helper) afterwards
    struct Wait {
      std::atomic<bool> &d;
      ~Wait() { while (!d.load(std::memory_order_acquire)) __builtin_ia32_pause(); }
    };
    {
      Wait w{done_};
      mine();
    }
    if (failed_.load()) throw std::runtime_error("host helper: the paired job threw");
  }

 private:
  void loop()
  {
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return wake_; });
        wake_ = false;
        if (quit_) return;
      }
      do {
        spinning_.store(true);
        auto until = std::chrono::steady_clock::now() + std::chrono::milliseconds(1);
        unsigned spins = 0;
        for (;;) {
          if (posted_.load(std::memory_order_acquire)) {
            posted_.store(false);
            try {
              (*job_)();
            } catch (...) {  // (bad_alloc of a result vector ...): reported by run_pair on the caller's thread
              failed_.store(true);
            }
            done_.store(true, std::memory_order_release);
            until = std::chrono::steady_clock::now() + std::chrono::milliseconds(1);
          } else {
            __builtin_ia32_pause();
            if ((++spins & 0xFF) == 0 && std::chrono::steady_clock::now() > until) break;
          }
        }
        spinning_.store(false);
      } while (posted_.load());  // posted while this thread was on its way to sleep: its poster saw `spinning_` and sent no wake
    }
  }
  std::once_flag started_;
  std::thread th_;
  std::mutex mu_, pair_mu_;
  std::condition_variable cv_;
  bool wake_ = false, quit_ = false;
  std::atomic<bool> spinning_{false}, posted_{false}, done_{false}, failed_{false};
  const std::function<void()> *job_ = nullptr;
};
std::atomic<int> g_host_threads{1};
HostHelper &host_helper()
{
  static HostHelper hh;
  return hh;
}

void host_helper_arm() { host_helper().arm(); }

static FleetWork g_ddp_work[64];      // mppi_compute_feedback_gains_batch -> ddp_fleet_kernel
static FleetWork g_nominal_work[64];  // mppi_nominal_traj_batch -> nominal_fleet_kernel
static FleetWork g_nominal_gains_work[64];  // mppi_nominal_and_gains_batch -> nominal_gains_fleet_kernel

// The sharing rule of the batched DDP pass, next to fleet_together: two or more handles of the network model with parameters set,
// all on one device.  Layer lists, T, hz, limits and weights may differ: they are data.  (The basis-function model stays on the
// host: its Jacobian is fp32 central differences through powf, which is ulp-sensitive.)
static bool ddp_fleet_together(mppi_handle *const *hs, int n)
{
  if (n < 2) return false;
  for (int i = 0; i < n; i++) {
    const mppi_handle *h = hs[i];
    if (h->basis || !h->have_nn || !image(h, Image::Theta) || !image(h, Image::Trace) || h->cfg.device != hs[0]->cfg.device) return false;
  }
  return true;
}

// n <= kMaxFleet handles of a ddp_fleet_together set: one launch.  xs / us: every handle's target sequences.  Returns MPPI_OK,
// MPPI_ERR_STATE when a handle's factorisation failed (that handle alone has no result), or the error that stopped the launch.
static int ddp_fleet_launch(mppi_handle *const *hs, const float *states, const float *const *xs, const float *const *us, int n)
{
  FleetPass p{hs, n, "batched DDP pass"};
  int rc = p.open(g_ddp_work, [&](int i) { return ddp_fleet_in_floats(hs[i]->T); }, [&](int i) { return ddp_fleet_out_floats(hs[i]->T); },
                  [&](int i) { return ddp_fleet_work_floats(hs[i]->T, hs[i]->net); }, [&](int i, float *in) {
    const int T = hs[i]->T;
    memcpy(in, states + (size_t)MPPI_STATE_DIM * i, sizeof(float) * kStateDim);
    memcpy(in + 7, xs[i], sizeof(float) * (size_t)T * kStateDim);
    memcpy(in + 7 + (size_t)7 * T, us[i], sizeof(float) * (size_t)T * kControlDim);
  });
  if (rc) return rc;
  for (int i = 0; i < n; i++) { hs[i]->have_ddp = false; hs[i]->ddp_on_device = 1; }
  p.launch(0, n, launch_ddp_fleet, [&](int i, DdpFleetArgs &a) {
    const mppi_handle *h = hs[i];
    a.theta = image(h, Image::Theta);
    a.wimg = image(h, Image::Trace);
    a.in = p.w->d_in + p.in_off[i];
    a.out = p.w->d_out + p.out_off[i];
    a.work = p.w->d_work + p.work_off[i];
    a.T = h->T;
    a.negate_yaw_der = h->cfg.negate_yaw_der ? 1 : 0;
    a.img_lds = ddp_fleet_image_in_lds(h->net) ? 1 : 0;
    a.dt = (float)(1.0 / h->cfg.hz);  // mppi_controller.cu:408
    for (int j = 0; j < kControlDim; j++) { a.u_lo[j] = h->u_lo[j]; a.u_hi[j] = h->u_hi[j]; a.R[j] = h->ddp_R[j]; }
    for (int q = 0; q < kStateDim; q++) { a.Q[q] = h->ddp_Q[q]; a.Qf[q] = h->ddp_Qf[q]; }
    a.net = h->net;
  });
  rc = p.finish();
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    mppi_handle *h = hs[i];
    const size_t T = (size_t)h->T;
    const float *o = p.w->h_out + p.out_off[i];
    int status = 0;
    memcpy(&status, o + 26 * T + 1, sizeof(int));
    if (status != 0) {
      rc = fail(h, MPPI_ERR_STATE, "DDP: control Hessian could not be factorised");
      continue;
    }
    DdpResult &r = h->ddp;
    r.feedback.assign(o, o + 14 * T);
    r.feedforward.assign(o + 14 * T, o + 16 * T);
    r.x.assign(o + 16 * T, o + 23 * T);
    r.u.assign(o + 23 * T, o + 25 * T);
    r.cost.assign(o + 25 * T, o + 26 * T);
    r.total_cost = o[26 * T];
    r.iterations = 1;
    h->have_ddp = true;
  }
  return rc;
}

// The sharing rule of the batched nominal replay, beside ddp_fleet_together: two or more handles of the network model with
// parameters set and a trace image, all on one device.  Everything else about a controller is data.  (The basis-function model
// stays on the host: its functions go through powf, which is ulp-sensitive -- the reason ddp_fleet_together gives.)
bool nominal_fleet_together(mppi_handle *const *hs, int n)
{
  if (n < 2) return false;
  for (int i = 0; i < n; i++) {
    const mppi_handle *h = hs[i];
    if (h->basis || !h->have_nn || !image(h, Image::Trace) || h->cfg.device != hs[0]->cfg.device) return false;
  }
  return true;
}

// The handles of a nominal_fleet_together set: one input copy, launches of up to kMaxFleet (each with its own slot of the argument
// ring), one result copy, one synchronise.  Inputs are every handle's HOST control sequence and the call's state; the caller's
// buffers are written only after EVERY launch has succeeded: an error leaves all of them as they were.
static int nominal_fleet_launch(mppi_handle *const *hs, const float *states, float *const *state_seqs, float *const *control_seqs, int n)
{
  FleetPass p{hs, n, "batched nominal replay"};
  int rc = p.open(g_nominal_work, [&](int i) { return nominal_fleet_in_floats(hs[i]->T); }, [&](int i) { return nominal_fleet_out_floats(hs[i]->T); },
                  [](int) { return (size_t)0; }, [&](int i, float *in) {
    memcpy(in, states + (size_t)MPPI_STATE_DIM * i, sizeof(float) * kStateDim);
    memcpy(in + 7, hs[i]->U.data(), sizeof(float) * (size_t)hs[i]->T * kControlDim);
  });
  if (rc) return rc;
  for (int at = 0; at < n; at += kMaxFleet)
    p.launch(at, std::min(kMaxFleet, n - at), launch_nominal_fleet, [&](int i, NominalFleetArgs &a) {
      const mppi_handle *h = hs[i];
      a.wimg = image(h, Image::Trace);
      a.in = p.w->d_in + p.in_off[i];
      a.out = p.w->d_out + p.out_off[i];
      a.T = h->T;
      a.negate_yaw_der = h->cfg.negate_yaw_der ? 1 : 0;
      a.img_lds = nominal_fleet_image_in_lds(h->net) ? 1 : 0;
      a.dt = h->dt;
      for (int j = 0; j < kControlDim; j++) { a.u_lo[j] = h->u_lo[j]; a.u_hi[j] = h->u_hi[j]; }
      a.net = h->net;
    });
  rc = p.finish();
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    const size_t T = (size_t)hs[i]->T;
    const float *o = p.w->h_out + p.out_off[i];
    memcpy(state_seqs[i], o, sizeof(float) * 7 * T);
    memcpy(control_seqs[i], o + 7 * T, sizeof(float) * 2 * T);
    hs[i]->nominal_on_device = 1;
  }
  return MPPI_OK;
}

// The handles of a set that is both nominal_fleet_together and ddp_fleet_together: every handle's replay and the DDP pass that
// tracks it in one workgroup of nominal_gains_fleet_kernel.  One input copy (the states and the HOST control sequences), launches
// of up to kMaxFleet, one result copy, one synchronise, as nominal_fleet_launch does it; the targets never come down in between.
// The caller's buffers and every handle's DDP result are written only after all of that has succeeded.  Returns MPPI_OK,
// MPPI_ERR_STATE when a handle's factorisation failed (that handle alone has no gains; its sequences are delivered), or the error
// that stopped the call.
static int nominal_gains_fleet_launch(mppi_handle *const *hs, const float *states, float *const *state_seqs, float *const *control_seqs,
                                      int n)
{
  FleetPass p{hs, n, "batched nominal replay and DDP pass"};
  int rc = p.open(g_nominal_gains_work, [&](int i) { return nominal_fleet_in_floats(hs[i]->T); },
                  [&](int i) { return nominal_gains_fleet_out_floats(hs[i]->T); },
                  [&](int i) { return ddp_fleet_work_floats(hs[i]->T, hs[i]->net); }, [&](int i, float *in) {
    memcpy(in, states + (size_t)MPPI_STATE_DIM * i, sizeof(float) * kStateDim);
    memcpy(in + 7, hs[i]->U.data(), sizeof(float) * (size_t)hs[i]->T * kControlDim);
  });
  if (rc) return rc;
  for (int at = 0; at < n; at += kMaxFleet)
    p.launch(at, std::min(kMaxFleet, n - at), launch_nominal_gains_fleet, [&](int i, NominalGainsFleetArgs &a) {
      const mppi_handle *h = hs[i];
      a.theta = image(h, Image::Theta);
      a.wimg = image(h, Image::Trace);
      a.in = p.w->d_in + p.in_off[i];
      a.out = p.w->d_out + p.out_off[i];
      a.work = p.w->d_work + p.work_off[i];
      a.T = h->T;
      a.negate_yaw_der = h->cfg.negate_yaw_der ? 1 : 0;
      a.img_lds = nominal_gains_fleet_image_in_lds(h->net) ? 1 : 0;
      a.dt = (float)(1.0 / h->cfg.hz);  // the pass's (ddp_fleet_launch)
      a.dt_nominal = h->dt;             // the replay's (nominal_fleet_launch)
      for (int j = 0; j < kControlDim; j++) { a.u_lo[j] = h->u_lo[j]; a.u_hi[j] = h->u_hi[j]; a.R[j] = h->ddp_R[j]; }
      for (int q = 0; q < kStateDim; q++) { a.Q[q] = h->ddp_Q[q]; a.Qf[q] = h->ddp_Qf[q]; }
      a.net = h->net;
    });
  rc = p.finish();
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    mppi_handle *h = hs[i];
    const size_t T = (size_t)h->T;
    const float *o = p.w->h_out + p.out_off[i];
    const float *seq = o + nominal_gains_fleet_seq_offset(h->T);
    memcpy(state_seqs[i], seq, sizeof(float) * 7 * T);
    memcpy(control_seqs[i], seq + 7 * T, sizeof(float) * 2 * T);
    h->nominal_on_device = h->ddp_on_device = h->nominal_gains_fused = 1;
    h->have_ddp = false;
    int status = 0;
    memcpy(&status, o + 26 * T + 1, sizeof(int));
    if (status != 0) {
      rc = fail(h, MPPI_ERR_STATE, "DDP: control Hessian could not be factorised");
      continue;
    }
    DdpResult &r = h->ddp;
    r.feedback.assign(o, o + 14 * T);
    r.feedforward.assign(o + 14 * T, o + 16 * T);
    r.x.assign(o + 16 * T, o + 23 * T);
    r.u.assign(o + 23 * T, o + 25 * T);
    r.cost.assign(o + 25 * T, o + 26 * T);
    r.total_cost = o[26 * T];
    r.iterations = 1;
    h->have_ddp = true;
  }
  return rc;
}

// ---- a plant of its own (mppi_set_plant_model, mppi_plant_drive_batch) ------------------------------------------------------------
static FleetWork g_plant_drive_work[64];  // mppi_plant_drive_batch -> plant_drive_fleet_kernel

const NetDesc &plant_net_of(const mppi_handle *h) { return h->have_plant ? h->plant_net : h->net; }
static int plant_negate_of(const mppi_handle *h) { return h->have_plant ? h->plant_negate : (h->cfg.negate_yaw_der ? 1 : 0); }
static const float *plant_image_of(const mppi_handle *h) { return h->have_plant ? h->d_plant_img : image(h, Image::Trace); }

// the largest image a layer list of mppi_create can have: 6 -> 256 x 6 -> 4
constexpr size_t kPlantImageMaxFloats = (size_t)(kNetIn + 1) * 256 + (size_t)(MPPI_MAX_LAYERS - 3) * 257 * 256 + (size_t)257 * kNetOut;

// Is a fitting image copied to LDS?  One step reads every weight once: the copy would be a second pass.  From two steps on the
// copy is read back `steps` times from LDS instead of from the L2.  MPPI_PLANT_DRIVE_LDS=0 / 1 (tools only, read at
// every call): never / whenever it fits -- tools/fleet_time.py --plant-drive measures the two.
static bool plant_drive_wants_lds(const NetDesc &net, int steps)
{
  if (!plant_drive_image_in_lds(net)) return false;
  if (const char *sw = getenv("MPPI_PLANT_DRIVE_LDS")) return atoi(sw) != 0;
  return steps >= 2;
}

void plant_drive_fill(const mppi_handle *h, int periods, int substeps, int feedback, PlantDriveArgs &a)
{
  a.wimg = plant_image_of(h);
  a.net = plant_net_of(h);
  a.negate_yaw_der = plant_negate_of(h);
  a.periods = periods;
  a.substeps = substeps;
  a.feedback = feedback ? 1 : 0;
  a.img_lds = plant_drive_wants_lds(a.net, periods * substeps) ? 1 : 0;
  a.dt_sub = h->dt / (float)substeps;
  for (int j = 0; j < kControlDim; j++) { a.u_lo[j] = h->u_lo[j]; a.u_hi[j] = h->u_hi[j]; }
  for (int j = 0; j < kPlantDriveMaxSubsteps; j++) a.a[j] = j < substeps ? (double)j / (double)substeps : 0.0;
}

// The drive law of include/mppi_hip.h on the host, statement for statement what plant_drive_fleet_kernel computes; only sinf /
// cosf of the heading are glibc's floats here and the rounded double results there.  model(s, u0, u1, sd): the plant's derivative
// rows 2 .. 6 (the yaw rate's sign and the dynamics); xs [.. periods + 1][7], us [.. periods + 1][2] the nominal solution; K
// [.. periods + 1][2][7] the gains or nullptr (no feedback); x_out [7]; applied [periods * substeps][2] or nullptr.
template <class Model>
static void plant_drive_host(Model &&model, float dt, const float *u_lo, const float *u_hi, const float *x0, const float *xs,
                             const float *us, const float *K, int periods, int substeps, float *x_out, float *applied)
{
  const int m = substeps;
  const float dt_sub = dt / (float)m;
  float s[kStateDim];
  for (int i = 0; i < kStateDim; i++) s[i] = x0[i];
  for (int q = 0; q < periods * m; q++) {
    const int lo = q / m, j = q % m, hi = lo + 1;
    double u[2];
    float xd[kStateDim], k[2 * kStateDim];
    if (j == 0) {  // nothing is interpolated: row hi is not read
      for (int c = 0; c < 2; c++) u[c] = (double)us[2 * lo + c];
      if (K) {
        for (int i = 0; i < kStateDim; i++) xd[i] = xs[7 * lo + i];
        for (int i = 0; i < 2 * kStateDim; i++) k[i] = K[14 * lo + i];
      }
    } else {
      const double a = (double)j / (double)m, b = 1.0 - a;
      for (int c = 0; c < 2; c++) u[c] = b * (double)us[2 * lo + c] + a * (double)us[2 * hi + c];
      if (K) {
        for (int i = 0; i < kStateDim; i++) xd[i] = (float)(b * (double)xs[7 * lo + i] + a * (double)xs[7 * hi + i]);
        for (int i = 0; i < 2 * kStateDim; i++) k[i] = (float)(b * (double)K[14 * lo + i] + a * (double)K[14 * hi + i]);
      }
    }
    if (K) {
      float du[2] = {0.0f, 0.0f};
      for (int c = 0; c < 2; c++)
        for (int i = 0; i < kStateDim; i++) du[c] = fmaf(k[7 * c + i], s[i] - xd[i], du[c]);
      if (!std::isnan(du[0]) && !std::isnan(du[1])) {  // autorally_plant.cpp:243-246: a NaN correction leaves the feed-forward
        u[0] += (double)du[0];
        u[1] += (double)du[1];
      }
    }
    float ap[2];
    for (int c = 0; c < 2; c++) {  // nom_clamp with the HANDLE's limits (the reference clamps to +-1)
      const float v = (float)u[c];
      ap[c] = v < u_lo[c] ? u_lo[c] : (v > u_hi[c] ? u_hi[c] : v);
    }
    if (applied) {
      applied[2 * q] = ap[0];
      applied[2 * q + 1] = ap[1];
    }
    const float c = cosf(s[2]), sn = sinf(s[2]);
    float sd[kStateDim];
    sd[0] = fmaf(c, s[4], -(sn * s[5]));
    sd[1] = fmaf(sn, s[4], c * s[5]);
    model(s, ap[0], ap[1], sd);
    for (int i = 0; i < kStateDim; i++) s[i] = fmaf(sd[i], dt_sub, s[i]);
  }
  for (int i = 0; i < kStateDim; i++) x_out[i] = s[i];
}

// the network plant: mppi_nominal_traj's statements
static auto net_plant(HostNetFma &net, int negate)
{
  return [&net, negate](const float *s, float u0, float u1, float *sd) {
    sd[2] = negate ? -s[6] : s[6];
    const float nin6[6] = {s[3], s[4], s[5], s[6], u0, u1};
    net.forward(nin6, sd + 3);
  };
}

// one handle's drive on the host: the plant set for it, or its own model (which may be the basis-function model)
static void plant_drive_host_handle(mppi_handle *h, const float *x0, const float *xs, const float *us, const float *K, int periods,
                                    int substeps, float *x_out, float *applied)
{
  if (h->basis) {  // GeneralizedLinear::updateState (generalized_linear.cu:140-167), yaw rate always negated
    plant_drive_host([h](const float *s, float u0, float u1, float *sd) {
      float phi[kNumBfs];
      sd[2] = -s[6];
      basis_funcs(s, u0, u1, phi);
      basis_dynamics(h->theta.data(), phi, sd + 3);
    }, h->dt, h->u_lo, h->u_hi, x0, xs, us, K, periods, substeps, x_out, applied);
    return;
  }
  plant_drive_host(net_plant(h->have_plant ? h->plant_hnet : h->hnet, plant_negate_of(h)), h->dt, h->u_lo, h->u_hi, x0, xs, us, K, periods,
                   substeps, x_out, applied);
}

// The sharing rule, as nominal_fleet_together: two or more handles of the network model with parameters set and a plant image,
// all on one device.  Layer lists (the controller's and the plant's), T, hz and limits are data.
bool plant_drive_together(mppi_handle *const *hs, int n)
{
  if (n < 2) return false;
  for (int i = 0; i < n; i++) {
    const mppi_handle *h = hs[i];
    if (h->basis || !h->have_nn || !plant_image_of(h) || h->cfg.device != hs[0]->cfg.device) return false;
  }
  return true;
}

static size_t drive_in_floats(int periods, int feedback)
{
  const size_t rows = (size_t)periods + 1;
  return 8 + align4(2 * rows) + (feedback ? align4(7 * rows) + 14 * rows : 0);
}

// The handles of a plant_drive_together set: one input copy (states, the first periods + 1 rows of the sequences and gains),
// launches of up to kMaxFleet, one result copy, one synchronise; the caller's buffers are written only after all of it succeeded.
static int plant_drive_launch(mppi_handle *const *hs, const float *states, const float *const *xs, const float *const *us, int n, int periods,
                              int substeps, int feedback, float *states_out, float *const *applied_log)
{
  const size_t rows = (size_t)periods + 1, steps = (size_t)periods * substeps;
  const size_t off_u = 8, off_x = off_u + align4(2 * rows), off_k = off_x + align4(7 * rows);
  FleetPass p{hs, n, "batched plant drive"};
  int rc = p.open(g_plant_drive_work, [&](int) { return drive_in_floats(periods, feedback); }, [&](int) { return 8 + 2 * steps; },
                  [](int) { return (size_t)0; }, [&](int i, float *in) {
    memcpy(in, states + (size_t)MPPI_STATE_DIM * i, sizeof(float) * kStateDim);
    in[7] = 0.0f;
    memcpy(in + off_u, us[i], sizeof(float) * 2 * rows);
    if (feedback) {
      memcpy(in + off_x, xs[i], sizeof(float) * 7 * rows);
      memcpy(in + off_k, hs[i]->ddp.feedback.data(), sizeof(float) * 14 * rows);
    }
  });
  if (rc) return rc;
  for (int at = 0; at < n; at += kMaxFleet)
    p.launch(at, std::min(kMaxFleet, n - at), +[](const PlantDriveArgs *h_inst, const PlantDriveArgs *d_inst, int m, hipStream_t S) {
      return launch_plant_drive_fleet(h_inst, d_inst, nullptr, m, 0, S);
    }, [&](int i, PlantDriveArgs &a) {
      plant_drive_fill(hs[i], periods, substeps, feedback, a);
      const float *in = p.w->d_in + p.in_off[i];
      float *out = p.w->d_out + p.out_off[i];
      a.useq_even = a.useq_odd = in + off_u;
      a.xseq = feedback ? in + off_x : nullptr;
      a.gains = feedback ? in + off_k : nullptr;
      a.state_in = in;
      a.state_out = out;
      a.applied = out + 8;
    });
  rc = p.finish();
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    const float *o = p.w->h_out + p.out_off[i];
    memcpy(states_out + (size_t)MPPI_STATE_DIM * i, o, sizeof(float) * kStateDim);
    if (applied_log && applied_log[i]) memcpy(applied_log[i], o + 8, sizeof(float) * 2 * steps);
    hs[i]->plant_drive_on_device = 1;
  }
  return MPPI_OK;
}

// a layer list mppi_create accepts; its parameter count
static bool plant_layers_ok(const int *layers, int n_layers, size_t *num_params)
{
  if (!layers || n_layers < 2 || n_layers > MPPI_MAX_LAYERS) return false;
  if (layers[0] != kNetIn || layers[n_layers - 1] != kNetOut) return false;
  size_t np = 0;
  for (int i = 0; i < n_layers; i++)
    if (layers[i] <= 0 || layers[i] > 256) return false;
  for (int i = 0; i + 1 < n_layers; i++) np += (size_t)(layers[i] + 1) * layers[i + 1];
  *num_params = np;
  return true;
}

static NetDesc net_desc_of(const int *layers, int n_layers, size_t num_params)
{
  NetDesc net{};
  net.n_layers = n_layers;
  for (int i = 0; i < 8; i++) net.layers[i] = i < n_layers ? layers[i] : 0;
  for (int i = 0; i < n_layers; i++) net.max_width = std::max(net.max_width, layers[i]);
  net.num_params = (int)num_params;
  return net;
}

}  // namespace mppi_abi

extern "C" {

int mppi_set_plant_model(mppi_handle *h, const int *layers, int n_layers, const float *theta, size_t n, int negate_yaw_der)
{
  if (!h) return MPPI_ERR_INVALID;
  if (h->basis) return fail(h, MPPI_ERR_INVALID, "a plant model is a network: the handle was created for basis-function dynamics");
  if (n_layers == 0 && theta == nullptr) {  // cleared: the plant is the handle's own network again (the image's memory is kept)
    h->have_plant = false;
    return MPPI_OK;
  }
  size_t np = 0;
  if (!theta || !plant_layers_ok(layers, n_layers, &np)) return fail(h, MPPI_ERR_INVALID, "plant model: the layer list must be 6 .. 4 with widths 1 .. 256");
  if (n != np) return fail(h, MPPI_ERR_INVALID, "plant model: theta size != NUM_PARAMS of the layer list");
  const NetDesc net = net_desc_of(layers, n_layers, np);
  const std::vector<float> th(theta, theta + n);
  const std::vector<float> img = pack_trace_weights(th, net);
  HIPCHK(h, ensure_device(h->cfg.device));
  // no solve state is touched and an armed handle stays armed: the copy goes to the device's batch stream, which no solve of a
  // single handle waits on, and no device memory is freed
  hipStream_t S = batch_stream(h->cfg.device);
  if (!S) return fail(h, MPPI_ERR_HIP, "no batch stream");
  float *d = h->d_plant_img;
  if (!d) HIPCHK(h, hipMalloc(reinterpret_cast<void **>(&d), sizeof(float) * kPlantImageMaxFloats));
  h->d_plant_img = d;
  hipError_t e = hipMemcpyAsync(d, img.data(), sizeof(float) * img.size(), hipMemcpyHostToDevice, S);
  if (e == hipSuccess) e = hipStreamSynchronize(S);
  if (e != hipSuccess) {  // the image may be half written: no plant model rather than a wrong one
    h->have_plant = false;
    return fail(h, MPPI_ERR_HIP, "plant model: image copy", e);
  }
  h->plant_net = net;
  h->plant_negate = negate_yaw_der ? 1 : 0;
  h->plant_theta = th;
  h->plant_hnet.init(h->plant_net.layers, h->plant_net.n_layers, h->plant_theta.data());
  h->have_plant = true;
  return MPPI_OK;
}

int mppi_debug_plant_model_info(const mppi_handle *h, int *n_layers)
{
  if (!h || !n_layers) return MPPI_ERR_INVALID;
  *n_layers = h->have_plant ? h->plant_net.n_layers : 0;
  return MPPI_OK;
}

int mppi_debug_plant_drive_host(const int *layers, int n_layers, const float *theta, size_t n, int negate_yaw_der, float dt,
                                const float u_lo[MPPI_CONTROL_DIM], const float u_hi[MPPI_CONTROL_DIM], const float x[MPPI_STATE_DIM],
                                const float *state_seq, const float *control_seq, const float *feedback, int T, int periods, int substeps,
                                float state_out[MPPI_STATE_DIM], float *applied)
{
  size_t np = 0;
  if (!theta || !u_lo || !u_hi || !x || !control_seq || !state_out || !plant_layers_ok(layers, n_layers, &np) || n != np) return MPPI_ERR_INVALID;
  if (feedback && !state_seq) return MPPI_ERR_INVALID;
  if (T < 2 || periods < 1 || periods >= T || substeps < 1 || substeps > kPlantDriveMaxSubsteps || !(dt > 0.0f)) return MPPI_ERR_INVALID;
  HostNetFma net;
  net.init(layers, n_layers, theta);
  plant_drive_host(net_plant(net, negate_yaw_der ? 1 : 0), dt, u_lo, u_hi, x, state_seq, control_seq, feedback, periods, substeps, state_out,
                   applied);
  return MPPI_OK;
}

int mppi_plant_drive_batch(mppi_handle *const *handles, const float *states, const float *const *state_seqs, const float *const *control_seqs,
                           int n, int periods, int substeps, int feedback, float *states_out, float *const *applied_log)
{
  // mppi_nominal_traj_batch's order: every argument, then every handle's readiness, then every pending solve; only then an output
  if (!handles || !states || !state_seqs || !control_seqs || !states_out || n < 1) return MPPI_ERR_INVALID;
  for (int i = 0; i < n; i++) {
    if (!handles[i] || !state_seqs[i] || !control_seqs[i]) return MPPI_ERR_INVALID;
    for (int q = 0; q < i; q++)
      if (handles[q] == handles[i]) return fail(handles[i], MPPI_ERR_INVALID, "the same handle twice in one batch");
  }
  if (substeps < 1 || substeps > kPlantDriveMaxSubsteps) return fail(handles[0], MPPI_ERR_INVALID, "plant drive: substeps must be in [1, 16]");
  for (int i = 0; i < n; i++)
    if (periods < 1 || periods >= handles[i]->T) return fail(handles[i], MPPI_ERR_INVALID, "plant drive: periods must be in [1, T)");
  for (int i = 0; i < n; i++)
    if (!handles[i]->have_nn) return fail(handles[i], MPPI_ERR_STATE, "mppi_set_nn_params has not been called");
  for (int i = 0; i < n && feedback; i++)
    if (!handles[i]->have_ddp) return fail(handles[i], MPPI_ERR_STATE, "plant drive with feedback: the handle has no DDP result");
  for (int i = 0; i < n; i++)
    if (handles[i]->pending) {
      const int rc = mppi_synchronize(handles[i]);
      if (rc) return rc;
    }
  if (plant_drive_together(handles, n))
    return plant_drive_launch(handles, states, state_seqs, control_seqs, n, periods, substeps, feedback, states_out, applied_log);
  // n host drives; every result is computed before one is delivered (states_out may be `states`)
  const size_t steps = (size_t)periods * substeps;
  std::vector<float> xo((size_t)MPPI_STATE_DIM * n), ap(2 * steps * (size_t)n);
  for (int i = 0; i < n; i++)
    plant_drive_host_handle(handles[i], states + (size_t)MPPI_STATE_DIM * i, state_seqs[i], control_seqs[i],
                            feedback ? handles[i]->ddp.feedback.data() : nullptr, periods, substeps, xo.data() + (size_t)MPPI_STATE_DIM * i,
                            ap.data() + 2 * steps * i);
  memcpy(states_out, xo.data(), sizeof(float) * xo.size());
  for (int i = 0; i < n; i++) {
    if (applied_log && applied_log[i]) memcpy(applied_log[i], ap.data() + 2 * steps * i, sizeof(float) * 2 * steps);
    handles[i]->plant_drive_on_device = 0;
  }
  return MPPI_OK;
}

int mppi_debug_plant_drive_info(const mppi_handle *h, int *on_device)
{
  if (!h || !on_device) return MPPI_ERR_INVALID;
  *on_device = h->plant_drive_on_device;
  return MPPI_OK;
}

int mppi_nominal_and_gains_batch(mppi_handle *const *handles, const float *states, float *const *state_seqs, float *const *control_seqs,
                                 int n)
{
  // mppi_nominal_traj_batch's order: every argument, then every handle's readiness, then every pending solve; only then a launch
  if (!handles || !states || !state_seqs || !control_seqs || n < 1) return MPPI_ERR_INVALID;
  for (int i = 0; i < n; i++) {
    if (!handles[i] || !state_seqs[i] || !control_seqs[i]) return MPPI_ERR_INVALID;
    for (int q = 0; q < i; q++)
      if (handles[q] == handles[i]) return fail(handles[i], MPPI_ERR_INVALID, "the same handle twice in one batch");
  }
  for (int i = 0; i < n; i++) handles[i]->nominal_gains_fused = 0;
  if (!nominal_fleet_together(handles, n) || !ddp_fleet_together(handles, n)) {
    // exactly the two calls, one after the other: their bits, their errors, their order of work
    const int rc = mppi_nominal_traj_batch(handles, states, state_seqs, control_seqs, n);
    if (rc) return rc;
    return mppi_compute_feedback_gains_batch(handles, states, state_seqs, control_seqs, n);
  }
  // (every handle of a shared set has its parameters: the sharing rules say so)
  for (int i = 0; i < n; i++)
    if (handles[i]->pending) {
      const int rc = mppi_synchronize(handles[i]);
      if (rc) return rc;
    }
  return nominal_gains_fleet_launch(handles, states, state_seqs, control_seqs, n);  // more than kMaxFleet handles: launches of up to kMaxFleet
}

int mppi_debug_nominal_and_gains_info(const mppi_handle *h, int *fused)
{
  if (!h || !fused) return MPPI_ERR_INVALID;
  *fused = h->nominal_gains_fused;
  return MPPI_OK;
}

int mppi_nominal_traj(mppi_handle *h, const float state[MPPI_STATE_DIM], float *state_seq, float *control_seq)
{
  if (!h || !state || !state_seq || !control_seq) return MPPI_ERR_INVALID;
  if (!h->have_nn) return fail(h, MPPI_ERR_STATE, "mppi_set_nn_params has not been called");
  if (h->pending) {
    int rc = mppi_synchronize(h);
    if (rc) return rc;
  }
  h->nominal_on_device = 0;
  // computeNominalTraj (mppi_controller.cu:501-519) -> host updateState (neural_net_model.cu:280-288):
  // like the reference this replay runs on the host (T sequential 1.4k-MAC steps).
  float s[kStateDim];
  for (int i = 0; i < kStateDim; i++) s[i] = state[i];
  for (int t = 0; t < h->T; t++) {
    for (int i = 0; i < kStateDim; i++) state_seq[t * kStateDim + i] = s[i];
    float u[2] = {h->U[2 * t], h->U[2 * t + 1]};
    for (int i = 0; i < 2; i++) {
      if (u[i] < h->u_lo[i]) u[i] = h->u_lo[i];
      else if (u[i] > h->u_hi[i]) u[i] = h->u_hi[i];
    }
    const float c = cosf(s[2]), sn = sinf(s[2]);
    float sd[kStateDim];
    sd[0] = fmaf(c, s[4], -(sn * s[5]));
    sd[1] = fmaf(sn, s[4], c * s[5]);
    sd[2] = h->cfg.negate_yaw_der ? -s[6] : s[6];
    if (h->basis) {  // GeneralizedLinear::updateState (generalized_linear.cu:140-167), yaw rate always negated
      float phi[kNumBfs];
      sd[2] = -s[6];
      basis_funcs(s, u[0], u[1], phi);
      basis_dynamics(h->theta.data(), phi, sd + 3);
      for (int i = 0; i < kStateDim; i++) s[i] = fmaf(sd[i], h->dt, s[i]);
      control_seq[2 * t] = u[0];
      control_seq[2 * t + 1] = u[1];
      continue;
    }
    // the network: per neuron the k-ascending fmaf chain, bias added afterwards, tanhf -- eight neurons per AVX2
    // register (host_net.hpp; the same values as the scalar loops, bit for bit)
    const float nin6[6] = {s[3], s[4], s[5], s[6], u[0], u[1]};
    h->hnet.forward(nin6, sd + 3);
    for (int i = 0; i < kStateDim; i++) s[i] = fmaf(sd[i], h->dt, s[i]);
    control_seq[2 * t] = u[0];
    control_seq[2 * t + 1] = u[1];
  }
  return MPPI_OK;
}

int mppi_nominal_traj_pair(mppi_handle *ha, const float state_a[MPPI_STATE_DIM], float *state_seq_a, float *control_seq_a,
                           mppi_handle *hb, const float state_b[MPPI_STATE_DIM], float *state_seq_b, float *control_seq_b)
{
  if (!ha || !hb || ha == hb) return MPPI_ERR_INVALID;
  // two network replays of the same length advance in lockstep (host_net_forward2); anything else: one after the other
  const bool lockstep = !ha->basis && !hb->basis && ha->have_nn && hb->have_nn && ha->T == hb->T &&
                        ha->net.n_layers == hb->net.n_layers &&
                        memcmp(ha->net.layers, hb->net.layers, sizeof(ha->net.layers)) == 0 && state_a && state_b &&
                        state_seq_a && state_seq_b && control_seq_a && control_seq_b;
  if (g_host_threads.load(std::memory_order_relaxed) >= 2) {  // one replay per thread (mppi_set_host_threads), any model
    for (mppi_handle *h : {ha, hb})
      if (h->pending) {
        const int rc = mppi_synchronize(h);
        if (rc) return rc;
      }
    int rca = MPPI_OK, rcb = MPPI_OK;
    try {
      host_helper().run_pair([&] { rcb = mppi_nominal_traj(hb, state_b, state_seq_b, control_seq_b); },
                             [&] { rca = mppi_nominal_traj(ha, state_a, state_seq_a, control_seq_a); });
    } catch (const std::exception &e) {
      return fail(ha, MPPI_ERR_HIP, e.what());
    }
    return rca ? rca : rcb;
  }
  if (!lockstep) {
    const int rc = mppi_nominal_traj(ha, state_a, state_seq_a, control_seq_a);
    return rc ? rc : mppi_nominal_traj(hb, state_b, state_seq_b, control_seq_b);
  }
  for (mppi_handle *h : {ha, hb})
    if (h->pending) {
      const int rc = mppi_synchronize(h);
      if (rc) return rc;
    }
  mppi_handle *hs[2] = {ha, hb};
  ha->nominal_on_device = hb->nominal_on_device = 0;
  float *sseq[2] = {state_seq_a, state_seq_b}, *cseq[2] = {control_seq_a, control_seq_b};
  float s[2][kStateDim], sd[2][kStateDim], in6[2][6];
  for (int i = 0; i < kStateDim; i++) { s[0][i] = state_a[i]; s[1][i] = state_b[i]; }
  for (int t = 0; t < ha->T; t++) {
    for (int q = 0; q < 2; q++) {  // per replay exactly the statements of mppi_nominal_traj
      const mppi_handle *h = hs[q];
      for (int i = 0; i < kStateDim; i++) sseq[q][t * kStateDim + i] = s[q][i];
      float u[2] = {h->U[2 * t], h->U[2 * t + 1]};
      for (int i = 0; i < 2; i++) {
        if (u[i] < h->u_lo[i]) u[i] = h->u_lo[i];
        else if (u[i] > h->u_hi[i]) u[i] = h->u_hi[i];
      }
      const float c = cosf(s[q][2]), sn = sinf(s[q][2]);
      sd[q][0] = fmaf(c, s[q][4], -(sn * s[q][5]));
      sd[q][1] = fmaf(sn, s[q][4], c * s[q][5]);
      sd[q][2] = h->cfg.negate_yaw_der ? -s[q][6] : s[q][6];
      in6[q][0] = s[q][3]; in6[q][1] = s[q][4]; in6[q][2] = s[q][5]; in6[q][3] = s[q][6]; in6[q][4] = u[0]; in6[q][5] = u[1];
      cseq[q][2 * t] = u[0];
      cseq[q][2 * t + 1] = u[1];
    }
    host_net_forward2(ha->hnet, hb->hnet, in6[0], in6[1], sd[0] + 3, sd[1] + 3);
    for (int q = 0; q < 2; q++)
      for (int i = 0; i < kStateDim; i++) s[q][i] = fmaf(sd[q][i], hs[q]->dt, s[q][i]);
  }
  return MPPI_OK;
}

int mppi_nominal_traj_batch(mppi_handle *const *handles, const float *states, float *const *state_seqs, float *const *control_seqs,
                            int n)
{
  // first pass: every argument, then every handle's readiness, then every pending solve; only then an output or a launch
  if (!handles || !states || !state_seqs || !control_seqs || n < 1) return MPPI_ERR_INVALID;
  for (int i = 0; i < n; i++) {
    if (!handles[i] || !state_seqs[i] || !control_seqs[i]) return MPPI_ERR_INVALID;
    for (int q = 0; q < i; q++)
      if (handles[q] == handles[i]) return fail(handles[i], MPPI_ERR_INVALID, "the same handle twice in one batch");
  }
  for (int i = 0; i < n; i++)
    if (!handles[i]->have_nn) return fail(handles[i], MPPI_ERR_STATE, "mppi_set_nn_params has not been called");
  for (int i = 0; i < n; i++)
    if (handles[i]->pending) {
      const int rc = mppi_synchronize(handles[i]);
      if (rc) return rc;
    }
  if (!nominal_fleet_together(handles, n)) {
    // n host replays, the bits of n single calls
    for (int i = 0; i < n; i++) {
      const int rc = mppi_nominal_traj(handles[i], states + (size_t)MPPI_STATE_DIM * i, state_seqs[i], control_seqs[i]);
      if (rc) return rc;
    }
    return MPPI_OK;
  }
  return nominal_fleet_launch(handles, states, state_seqs, control_seqs, n);  // more than kMaxFleet handles: launches of up to kMaxFleet
}

int mppi_debug_nominal_info(const mppi_handle *h, int *on_device)
{
  if (!h || !on_device) return MPPI_ERR_INVALID;
  *on_device = h->nominal_on_device;
  return MPPI_OK;
}

int mppi_set_ddp_weights(mppi_handle *h, const float Q[MPPI_STATE_DIM], const float R[MPPI_CONTROL_DIM],
                         const float Qf[MPPI_STATE_DIM])
{
  if (!h || !Q || !R || !Qf) return MPPI_ERR_INVALID;
  for (int i = 0; i < kStateDim; i++) {
    if (!(Q[i] >= 0.0f) || !(Qf[i] >= 0.0f)) return fail(h, MPPI_ERR_INVALID, "Q and Qf must be non-negative");
  }
  for (int j = 0; j < kControlDim; j++)
    if (!(R[j] > 0.0f)) return fail(h, MPPI_ERR_INVALID, "R must be positive");
  memcpy(h->ddp_Q, Q, sizeof(h->ddp_Q));
  memcpy(h->ddp_R, R, sizeof(h->ddp_R));
  memcpy(h->ddp_Qf, Qf, sizeof(h->ddp_Qf));
  return MPPI_OK;
}

int mppi_compute_feedback_gains(mppi_handle *h, const float state[MPPI_STATE_DIM],
                                const float *target_state_seq, const float *target_control_seq)
{
  if (!h || !state) return MPPI_ERR_INVALID;
  if ((target_state_seq == nullptr) != (target_control_seq == nullptr))
    return fail(h, MPPI_ERR_INVALID, "give both target sequences or neither");
  if (!h->have_nn) return fail(h, MPPI_ERR_STATE, "mppi_set_nn_params has not been called");
  const int T = h->T;
  std::vector<float> xs((size_t)T * kStateDim), us((size_t)T * kControlDim);
  if (target_state_seq) {
    memcpy(xs.data(), target_state_seq, sizeof(float) * xs.size());
    memcpy(us.data(), target_control_seq, sizeof(float) * us.size());
  } else {
    int rc = mppi_nominal_traj(h, state, xs.data(), us.data());  // state_solution_, control_solution_
    if (rc) return rc;
  }
  DdpNet net;
  net.n_layers = h->basis ? 0 : h->net.n_layers;  // 0: basis-function model, theta = W[4][25]
  net.layers = h->net.layers;
  net.theta = h->theta.data();
  net.max_width = h->net.max_width;
  DdpProblem p;
  p.T = T;
  p.dt = (float)(1.0 / h->cfg.hz);  // mppi_controller.cu:408
  for (int j = 0; j < kControlDim; j++) { p.u_lo[j] = h->u_lo[j]; p.u_hi[j] = h->u_hi[j]; p.R[j] = h->ddp_R[j]; }
  for (int i = 0; i < kStateDim; i++) { p.Q[i] = h->ddp_Q[i]; p.Qf[i] = h->ddp_Qf[i]; }
  p.negate_yaw_der = h->cfg.negate_yaw_der;
  h->have_ddp = false;
  h->ddp_on_device = 0;
  if (ddp_feedback_gains(net, p, state, xs.data(), us.data(), h->ddp) != 0)
    return fail(h, MPPI_ERR_STATE, "DDP: control Hessian could not be factorised");
  h->have_ddp = true;
  return MPPI_OK;
}

int mppi_compute_feedback_gains_pair(mppi_handle *ha, const float state_a[MPPI_STATE_DIM], const float *target_state_seq_a,
                                     const float *target_control_seq_a, mppi_handle *hb, const float state_b[MPPI_STATE_DIM],
                                     const float *target_state_seq_b, const float *target_control_seq_b)
{
  if (!ha || !hb || ha == hb) return MPPI_ERR_INVALID;
  if (g_host_threads.load(std::memory_order_relaxed) >= 2) {
    // the nominal replays inside (no targets given) synchronise their handle: do that on this thread, which has the device
    for (mppi_handle *h : {ha, hb})
      if (h->pending) {
        const int rc = mppi_synchronize(h);
        if (rc) return rc;
      }
    int rca = MPPI_OK, rcb = MPPI_OK;
    try {  // no exception crosses the ABI: one thrown on either thread (an allocation of the result vectors) becomes a status
      host_helper().run_pair([&] { rcb = mppi_compute_feedback_gains(hb, state_b, target_state_seq_b, target_control_seq_b); },
                             [&] { rca = mppi_compute_feedback_gains(ha, state_a, target_state_seq_a, target_control_seq_a); });
    } catch (const std::exception &e) {
      return fail(ha, MPPI_ERR_HIP, e.what());
    }
    return rca ? rca : rcb;
  }
  const int rc = mppi_compute_feedback_gains(ha, state_a, target_state_seq_a, target_control_seq_a);
  return rc ? rc : mppi_compute_feedback_gains(hb, state_b, target_state_seq_b, target_control_seq_b);
}

int mppi_compute_feedback_gains_batch(mppi_handle *const *handles, const float *states, const float *const *target_state_seqs,
                                      const float *const *target_control_seqs, int n)
{
  if (!handles || !states || n < 1) return MPPI_ERR_INVALID;
  for (int i = 0; i < n; i++) {
    if (!handles[i]) return MPPI_ERR_INVALID;
    for (int q = 0; q < i; q++)
      if (handles[q] == handles[i]) return fail(handles[i], MPPI_ERR_INVALID, "the same handle twice in one batch");
  }
  auto target = [n](const float *const *seqs, int i) -> const float * { return (seqs && i < n) ? seqs[i] : nullptr; };
  for (int i = 0; i < n; i++)
    if ((target(target_state_seqs, i) == nullptr) != (target(target_control_seqs, i) == nullptr))
      return fail(handles[i], MPPI_ERR_INVALID, "give both target sequences or neither");
  if (!ddp_fleet_together(handles, n)) {
    // n host passes, the bits of n single calls; every handle is tried, the first error is the call's
    int rc = MPPI_OK;
    for (int i = 0; i < n; i++) {
      const int rci = mppi_compute_feedback_gains(handles[i], states + (size_t)MPPI_STATE_DIM * i, target(target_state_seqs, i),
                                                  target(target_control_seqs, i));
      if (rci && !rc) rc = rci;
    }
    return rc;
  }
  // targets: the caller's, or the handle's nominal trajectory from the host replay, as in the single call
  std::vector<std::vector<float>> own_x(n), own_u(n);
  std::vector<const float *> xs(n), us(n);
  for (int i = 0; i < n; i++) {
    xs[i] = target(target_state_seqs, i);
    us[i] = target(target_control_seqs, i);
    if (xs[i]) continue;
    mppi_handle *h = handles[i];
    own_x[i].resize((size_t)h->T * kStateDim);
    own_u[i].resize((size_t)h->T * kControlDim);
    const int rc = mppi_nominal_traj(h, states + (size_t)MPPI_STATE_DIM * i, own_x[i].data(), own_u[i].data());
    if (rc) return rc;
    xs[i] = own_x[i].data();
    us[i] = own_u[i].data();
  }
  int rc = MPPI_OK;
  for (int at = 0; at < n; at += kMaxFleet) {  // more than kMaxFleet handles: launches of up to kMaxFleet
    const int m = std::min(kMaxFleet, n - at);
    const int rcm = ddp_fleet_launch(handles + at, states + (size_t)MPPI_STATE_DIM * at, xs.data() + at, us.data() + at, m);
    if (rcm == MPPI_ERR_HIP) return rcm;
    if (rcm && !rc) rc = rcm;
  }
  return rc;
}

int mppi_debug_ddp_info(const mppi_handle *h, int *on_device)
{
  if (!h || !on_device) return MPPI_ERR_INVALID;
  *on_device = h->ddp_on_device;
  return MPPI_OK;
}

int mppi_debug_device_tanhf(int device, const float *in, float *out, size_t n)
{
  if (device < 0 || !in || !out || n == 0) return MPPI_ERR_INVALID;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) return MPPI_ERR_NO_DEVICE;
  if (ensure_device(device) != hipSuccess) return MPPI_ERR_HIP;
  float *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_in), sizeof(float) * n);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_out), sizeof(float) * n);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, sizeof(float) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_device_tanhf(d_in, d_out, n, nullptr);
  if (e == hipSuccess) e = hipMemcpy(out, d_out, sizeof(float) * n, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return e == hipSuccess ? MPPI_OK : MPPI_ERR_HIP;
}

int mppi_set_host_threads(int n)
{
  if (n < 1 || n > 2) return MPPI_ERR_INVALID;
  g_host_threads.store(n, std::memory_order_relaxed);
  if (n >= 2) host_helper().arm();  // starts the helper now, not inside the first tick
  return MPPI_OK;
}

int mppi_get_feedback_gains(mppi_handle *h, float *feedback, float *feedforward, float *state_traj,
                            float *control_traj, float *total_cost)
{
  if (!h) return MPPI_ERR_INVALID;
  if (!h->have_ddp) return fail(h, MPPI_ERR_STATE, "mppi_compute_feedback_gains has not succeeded yet");
  const DdpResult &r = h->ddp;
  if (feedback) memcpy(feedback, r.feedback.data(), sizeof(float) * r.feedback.size());
  if (feedforward) memcpy(feedforward, r.feedforward.data(), sizeof(float) * r.feedforward.size());
  if (state_traj) memcpy(state_traj, r.x.data(), sizeof(float) * r.x.size());
  if (control_traj) memcpy(control_traj, r.u.data(), sizeof(float) * r.u.size());
  if (total_cost) *total_cost = r.total_cost;
  return MPPI_OK;
}

}  // extern "C"
