// abi_trace.hip -- mppi_trace_rollouts / mppi_top_rollouts: chosen rollouts of the most recent solve replayed on the device
// (rollout_trace.hip) from that solve's vehicle state and its applied controls, with the records no rollout kernel keeps.
// Follows mppi_get_applied_controls: a pending solve is collected first; while the handle is armed the work goes to the
// generator stream behind ev_arm -- in front of the gated kernels, not behind them -- and the handle stays armed.  Nothing is
// allocated, freed or uploaded here (hipFree waits for the device, gated kernels included): the records of a chunk of rollouts
// live in h->d_trace, its indices in host-mapped memory, both allocated with the handle; a call of more rollouts than a chunk
// is several launches.
//
// mppi_trace_rollouts_batch: the same for a whole fleet in one call.  Where the sharing rule holds (trace_fleet_together) the
// members' "best n" are chosen on the device (trace_select_fleet_kernel), the network members are traced in one launch per
// kMaxFleet (rollout_trace_fleet_kernel), the basis-function members in one of their own (rollout_trace_fleet_bf_kernel), all on
// the device's batch stream through one FleetPass: one input copy (the explicit indices), one result copy (only the outputs
// that were asked for), one synchronise.  Anything else is the per-handle calls above, one handle after the other.
#include "abi_internal.hpp"

#include <algorithm>
#include <numeric>

using namespace mppi;
using namespace mppi_abi;

namespace {

// the last solve exists and its result can be read: not lost, not before the first (a pending one has been collected)
int last_solve_there(mppi_handle *h)
{
  if (h->no_result) return fail(h, MPPI_ERR_HIP, "the last solve timed out: no result");
  if (!h->have_solve) return fail(h, MPPI_ERR_STATE, "no solve yet");
  return MPPI_OK;
}

int last_solve_ready(mppi_handle *h)
{
  int rc = mppi_synchronize(h);
  if (rc) return rc;
  return last_solve_there(h);
}

int no_weights(mppi_handle *h) { return fail(h, MPPI_ERR_STATE, "no solve yet (mppi_rollout_only computes no weights)"); }

// the cost outputs of a handle whose control cost is on (fill_cost_args: a non-zero coefficient, or an exploration_std whose square
// is not a finite non-zero number) are refused
int refuse_cost_outputs(mppi_handle *h)
{
  const bool coeff = h->cost.steering_coeff != 0.0f || h->cost.throttle_coeff != 0.0f;
  return fail(h, MPPI_ERR_UNSUPPORTED,
              coeff ? "a control cost is on: du = eps nu is not recoverable from the applied controls bit for bit (states, controls and "
                      "first_crash are served)"
                    : "exploration_std is zero or not finite, so the control-cost term is not an exact 0, and du = eps nu is not "
                      "recoverable from the applied controls (states, controls and first_crash are served)");
}

// everything of a trace launch that is the handle's: the last solve's state and applied controls, the current model, cost, costmap
// and limits.  The caller adds the indices, their number and the outputs.
void fill_trace_args(const mppi_handle *h, TraceArgs &a)
{
  fill_cost_args(h, a.cost);
  for (int i = 0; i < kStateDim; i++) a.state[i] = h->solve_state[i];
  a.V = h->v_buf;
  a.wimg = image(h, h->basis ? Image::Theta : Image::Trace);
  a.inv_t = h->d_invt;
  a.K = h->K;
  a.T = h->T;
  for (int i = 0; i < 2; i++) {
    a.nu[i] = h->cfg.exploration_std[i];
    a.u_lo[i] = h->u_lo[i];
    a.u_hi[i] = h->u_hi[i];
  }
  a.dt = h->dt;
  a.negate_yaw_der = h->cfg.negate_yaw_der ? 1 : 0;
}

FleetWork g_trace_work[64];  // mppi_trace_rollouts_batch -> trace_select_fleet_kernel, rollout_trace_fleet_kernel, rollout_trace_fleet_bf_kernel

// The sharing rule of the batched trace, beside nominal_fleet_together: two or more handles on one device, none armed (handles
// armed together wait gated on the batch stream, where this work would queue behind their gate; the per-handle call goes in front
// of its own), every count within one chunk and within the handle's K.  Model, layer list, K, T, scene and limits are data.
bool trace_fleet_together(mppi_handle *const *hs, const int *counts, int n)
{
  if (n < 2) return false;
  for (int i = 0; i < n; i++) {
    const mppi_handle *h = hs[i];
    if (h->cfg.device != hs[0]->cfg.device || h->armed || counts[i] > std::min(h->K, kTraceChunk)) return false;
    if (!image(h, h->basis ? Image::Theta : Image::Trace)) return false;
  }
  return true;
}

// one member of a fleet's trace: the caller's entry `at`, its rollouts, its indices (nullptr: the c largest weights)
struct TraceMember {
  mppi_handle *h;
  int at, c;
  const int *ks;
};
// which outputs the call asked for, and where a member's lie in its piece of the result buffer (float offsets; every record is 4 bytes)
struct TraceOutputs {
  bool states, controls, step_costs, costs, first_crash, ks;
};
struct TracePiece {
  size_t states, controls, step_costs, costs, first_crash, ks, total;
};
TracePiece trace_piece(const TraceOutputs &o, const TraceMember &m)
{
  const size_t c = (size_t)m.c, ct = c * (size_t)m.h->T;
  TracePiece p{};
  size_t at = 0;
  p.states = at;      at += o.states ? ct * kStateDim : 0;
  p.controls = at;    at += o.controls ? ct * kControlDim : 0;
  p.step_costs = at;  at += o.step_costs ? ct : 0;
  p.costs = at;       at += o.costs ? c : 0;
  p.first_crash = at; at += o.first_crash ? c : 0;
  p.ks = at;          at += (o.ks && !m.ks) ? c : 0;  // chosen on the device: they come back with the records
  p.total = at;
  return p;
}

// The members of a trace_fleet_together set with a count above 0, the network members first (n_net of them), every readiness check
// passed: select, trace, one result copy.  The caller's buffers are written only after everything has succeeded.
int trace_fleet_launch(const std::vector<TraceMember> &ms, int n_net, const TraceOutputs &o, int *const *ks_out, float *const *states,
                       float *const *controls, float *const *step_costs, float *const *costs, int *const *first_crash)
{
  const int n = (int)ms.size();
  std::vector<mppi_handle *> hs((size_t)n);
  std::vector<TracePiece> piece((size_t)n);
  bool any_top = false;
  for (int i = 0; i < n; i++) {
    hs[i] = ms[i].h;
    piece[i] = trace_piece(o, ms[i]);
    any_top = any_top || !ms[i].ks;
  }
  FleetPass p{hs.data(), n, "batched trace"};
  int rc = p.open(g_trace_work, [&](int i) { return (size_t)ms[i].c; }, [&](int i) { return piece[i].total; }, [](int) { return (size_t)0; },
                  [&](int i, float *in) {  // the device index array: a member's own indices, or room for the chosen ones
                    if (ms[i].ks) memcpy(in, ms[i].ks, sizeof(int) * (size_t)ms[i].c);
                    else memset(in, 0, sizeof(int) * (size_t)ms[i].c);
                  });
  if (rc) return rc;
  // what the kernels read of a handle (applied controls, weights) was written on the stream of its last solve: the handle's own,
  // unless the fleet solved together on this one
  for (int i = 0; i < n; i++)
    if (work_stream(hs[i]) != p.S) HIPCHK(hs[i], hipStreamSynchronize(work_stream(hs[i])));
  auto ks_of = [&](int i) { return reinterpret_cast<int *>(p.w->d_in + p.in_off[i]); };
  auto out_of = [&](int i) { return p.w->d_out + p.out_off[i]; };
  if (any_top)
    for (int at = 0; at < n; at += kMaxFleet)
      p.launch(at, std::min(kMaxFleet, n - at), launch_trace_select_fleet, [&](int i, TraceSelectArgs &s) {
        if (ms[i].ks) return;  // its indices are staged
        s.w = hs[i]->d_w;
        s.ks = ks_of(i);
        s.ks_out = o.ks ? reinterpret_cast<int *>(out_of(i) + piece[i].ks) : nullptr;
        s.K = hs[i]->K;
        s.n = ms[i].c;
      });
  auto fill = [&](int i, TraceFleetArgs &f) {
    const mppi_handle *h = hs[i];
    fill_trace_args(h, f.a);
    float *out = out_of(i);
    f.a.ks = ks_of(i);
    f.a.n = ms[i].c;
    f.a.states = o.states ? out + piece[i].states : nullptr;
    f.a.controls = o.controls ? out + piece[i].controls : nullptr;
    f.a.step_costs = o.step_costs ? out + piece[i].step_costs : nullptr;
    f.a.costs = o.costs ? out + piece[i].costs : nullptr;
    f.a.first_crash = o.first_crash ? reinterpret_cast<int *>(out + piece[i].first_crash) : nullptr;
    if (!h->basis) {
      f.net = h->net;
      f.img_lds = trace_image_in_lds(h->net) ? 1 : 0;
    }
  };
  for (int at = 0; at < n_net; at += kMaxFleet) p.launch(at, std::min(kMaxFleet, n_net - at), launch_rollout_trace_fleet, fill);
  for (int at = n_net; at < n; at += kMaxFleet) p.launch(at, std::min(kMaxFleet, n - at), launch_rollout_trace_fleet_bf, fill);
  rc = p.finish();
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    const TraceMember &m = ms[i];
    const size_t c = (size_t)m.c, ct = c * (size_t)m.h->T;
    const float *out = p.w->h_out + p.out_off[i];
    if (o.states) memcpy(states[m.at], out + piece[i].states, sizeof(float) * ct * kStateDim);
    if (o.controls) memcpy(controls[m.at], out + piece[i].controls, sizeof(float) * ct * kControlDim);
    if (o.step_costs) memcpy(step_costs[m.at], out + piece[i].step_costs, sizeof(float) * ct);
    if (o.costs) memcpy(costs[m.at], out + piece[i].costs, sizeof(float) * c);
    if (o.first_crash) memcpy(first_crash[m.at], out + piece[i].first_crash, sizeof(int) * c);
    if (o.ks) memcpy(ks_out[m.at], m.ks ? static_cast<const void *>(m.ks) : static_cast<const void *>(out + piece[i].ks), sizeof(int) * c);
  }
  return MPPI_OK;
}

}  // namespace

extern "C" {

int mppi_trace_rollouts(mppi_handle *h, const int *ks, int n, float *states, float *controls, float *step_costs,
                        float *costs, int *first_crash)
{
  if (!h) return MPPI_ERR_INVALID;
  if (n < 0) return fail(h, MPPI_ERR_INVALID, "n < 0");
  if (n > 0 && !ks) return fail(h, MPPI_ERR_INVALID, "ks is NULL");
  int rc = last_solve_ready(h);
  if (rc) return rc;
  for (int i = 0; i < n; i++)
    if (ks[i] < 0 || ks[i] >= h->K) return fail(h, MPPI_ERR_INVALID, "rollout index outside [0, K)");
  if (n == 0) return MPPI_OK;
  rc = check_ready(h);
  if (rc) return rc;
  TraceArgs a;
  fill_trace_args(h, a);
  if (a.cost.need_control_cost && (step_costs || costs)) return refuse_cost_outputs(h);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t S = h->stream;
  if (h->armed) {
    S = h->gstream;
    HIPCHK(h, hipStreamWaitEvent(S, h->ev_arm, 0));
  } else {
    OWN(h);
  }
  h->trace_on_device = 0;
  const int T = h->T, chunk = h->trace_chunk;
  // the chunk's records in h->d_trace
  float *d_states = h->d_trace;
  float *d_controls = d_states + (size_t)chunk * T * kStateDim;
  float *d_step = d_controls + (size_t)chunk * T * kControlDim;
  float *d_costs = d_step + (size_t)chunk * T;
  int *d_first = reinterpret_cast<int *>(d_costs + chunk);
  a.ks = h->d_trace_ks;
  a.states = states ? d_states : nullptr;
  a.controls = controls ? d_controls : nullptr;
  a.step_costs = step_costs ? d_step : nullptr;
  a.costs = costs ? d_costs : nullptr;
  a.first_crash = first_crash ? d_first : nullptr;
  for (int i0 = 0; i0 < n; i0 += chunk) {
    const int c = std::min(chunk, n - i0);
    a.n = c;
    memcpy(h->h_trace_ks, ks + i0, sizeof(int) * (size_t)c);  // host-mapped: the kernel reads it in place
    HIPCHK(h, h->basis ? launch_rollout_trace_bf(a, S) : launch_rollout_trace(h->net, a, S));
    const size_t ct = (size_t)c * T, at = (size_t)i0 * T;
    if (states) HIPCHK(h, hipMemcpyAsync(states + at * kStateDim, d_states, sizeof(float) * ct * kStateDim, hipMemcpyDeviceToHost, S));
    if (controls) HIPCHK(h, hipMemcpyAsync(controls + at * kControlDim, d_controls, sizeof(float) * ct * kControlDim, hipMemcpyDeviceToHost, S));
    if (step_costs) HIPCHK(h, hipMemcpyAsync(step_costs + at, d_step, sizeof(float) * ct, hipMemcpyDeviceToHost, S));
    if (costs) HIPCHK(h, hipMemcpyAsync(costs + i0, d_costs, sizeof(float) * (size_t)c, hipMemcpyDeviceToHost, S));
    if (first_crash) HIPCHK(h, hipMemcpyAsync(first_crash + i0, d_first, sizeof(int) * (size_t)c, hipMemcpyDeviceToHost, S));
    HIPCHK(h, hipStreamSynchronize(S));  // before the next chunk's indices and records replace these
  }
  return MPPI_OK;
}

int mppi_top_rollouts(mppi_handle *h, int n, int *ks)
{
  if (!h) return MPPI_ERR_INVALID;
  if (n < 0 || n > h->K) return fail(h, MPPI_ERR_INVALID, "n outside [0, K]");
  if (n > 0 && !ks) return fail(h, MPPI_ERR_INVALID, "ks is NULL");
  int rc = last_solve_ready(h);
  if (rc) return rc;
  if (!h->have_weights) return no_weights(h);
  if (n == 0) return MPPI_OK;
  std::vector<float> w((size_t)h->K);
  rc = mppi_get_results(h, nullptr, nullptr, nullptr, w.data());
  if (rc) return rc;
  std::vector<int> idx((size_t)h->K);
  std::iota(idx.begin(), idx.end(), 0);
  // descending weight, ties to the lower index; NaN weights (no completed solve has any) behind every number, by index
  std::partial_sort(idx.begin(), idx.begin() + n, idx.end(), [&](int x, int y) {
    const bool nx = std::isnan(w[x]), ny = std::isnan(w[y]);
    if (nx || ny) return nx == ny ? x < y : ny;
    return w[x] > w[y] || (w[x] == w[y] && x < y);
  });
  std::copy(idx.begin(), idx.begin() + n, ks);
  return MPPI_OK;
}

int mppi_trace_rollouts_batch(mppi_handle *const *handles, int n_handles, const int *counts, const int *const *ks, int *const *ks_out,
                              float *const *states, float *const *controls, float *const *step_costs, float *const *costs,
                              int *const *first_crash)
{
  // every argument first; then every pending solve; then every handle's readiness and the control-cost rule; only then a launch
  if (!handles || !counts || n_handles < 1) return MPPI_ERR_INVALID;
  const int n = n_handles;
  for (int i = 0; i < n; i++) {
    if (!handles[i]) return MPPI_ERR_INVALID;
    for (int q = 0; q < i; q++)
      if (handles[q] == handles[i]) return fail(handles[i], MPPI_ERR_INVALID, "the same handle twice in one batch");
  }
  auto ks_of = [&](int i) -> const int * { return ks ? ks[i] : nullptr; };
  for (int i = 0; i < n; i++) {
    mppi_handle *h = handles[i];
    const int c = counts[i];
    if (c < 0) return fail(h, MPPI_ERR_INVALID, "a negative count");
    if (c == 0) continue;
    if (const int *k = ks_of(i)) {
      for (int j = 0; j < c; j++)
        if (k[j] < 0 || k[j] >= h->K) return fail(h, MPPI_ERR_INVALID, "rollout index outside [0, K)");
    } else if (c > h->K) {
      return fail(h, MPPI_ERR_INVALID, "a count above K for the largest weights");
    }
    if ((ks_out && !ks_out[i]) || (states && !states[i]) || (controls && !controls[i]) || (step_costs && !step_costs[i]) ||
        (costs && !costs[i]) || (first_crash && !first_crash[i]))
      return fail(h, MPPI_ERR_INVALID, "an output array is given, but this handle's entry is NULL");
  }
  for (int i = 0; i < n; i++) {
    const int rc = mppi_synchronize(handles[i]);
    if (rc) return rc;
  }
  for (int i = 0; i < n; i++) {
    mppi_handle *h = handles[i];
    int rc = last_solve_there(h);
    if (rc) return rc;
    if (!ks_of(i) && !h->have_weights) return no_weights(h);
    if (counts[i] == 0) continue;
    rc = check_ready(h);
    if (rc) return rc;
  }
  if (step_costs || costs)
    for (int i = 0; i < n; i++) {
      CostArgs c;
      fill_cost_args(handles[i], c);
      if (counts[i] > 0 && c.need_control_cost) return refuse_cost_outputs(handles[i]);
    }
  if (!trace_fleet_together(handles, counts, n)) {
    // n per-handle calls, with their bits and errors
    for (int i = 0; i < n; i++) {
      mppi_handle *h = handles[i];
      const int c = counts[i];
      std::vector<int> top;
      const int *k = ks_of(i);
      if (!k && c > 0) {
        top.resize((size_t)c);
        const int rc = mppi_top_rollouts(h, c, top.data());
        if (rc) return rc;
        k = top.data();
      }
      const int rc = mppi_trace_rollouts(h, k, c, states ? states[i] : nullptr, controls ? controls[i] : nullptr,
                                         step_costs ? step_costs[i] : nullptr, costs ? costs[i] : nullptr, first_crash ? first_crash[i] : nullptr);
      if (rc) return rc;
      h->trace_on_device = 0;
      if (ks_out && c > 0) memcpy(ks_out[i], k, sizeof(int) * (size_t)c);
    }
    return MPPI_OK;
  }
  // the members with rollouts to trace, the network model's first
  std::vector<TraceMember> ms;
  for (int pass = 0; pass < 2; pass++)
    for (int i = 0; i < n; i++)
      if (counts[i] > 0 && handles[i]->basis == (pass == 1)) ms.push_back(TraceMember{handles[i], i, counts[i], ks_of(i)});
  int n_net = 0;
  for (const TraceMember &m : ms) n_net += m.h->basis ? 0 : 1;
  if (!ms.empty()) {
    const TraceOutputs o{states != nullptr, controls != nullptr, step_costs != nullptr, costs != nullptr, first_crash != nullptr, ks_out != nullptr};
    const int rc = trace_fleet_launch(ms, n_net, o, ks_out, states, controls, step_costs, costs, first_crash);
    if (rc) return rc;
  }
  for (int i = 0; i < n; i++) handles[i]->trace_on_device = 1;
  return MPPI_OK;
}

int mppi_debug_trace_info(const mppi_handle *h, int *on_device)
{
  if (!h || !on_device) return MPPI_ERR_INVALID;
  *on_device = h->trace_on_device;
  return MPPI_OK;
}

}  // extern "C"
