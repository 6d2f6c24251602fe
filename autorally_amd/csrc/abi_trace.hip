// abi_trace.hip -- mppi_trace_rollouts / mppi_top_rollouts: chosen rollouts of the most recent solve replayed on the device
// (rollout_trace.hip) from that solve's vehicle state and its applied controls, with the records no rollout kernel keeps.
// Follows mppi_get_applied_controls: a pending solve is collected first; while the handle is armed the work goes to the
// generator stream behind ev_arm -- in front of the gated kernels, not behind them -- and the handle stays armed.  Nothing is
// allocated, freed or uploaded here (hipFree waits for the device, gated kernels included): the records of a chunk of rollouts
// live in h->d_trace, its indices in host-mapped memory, both allocated with the handle; a call of more rollouts than a chunk
// is several launches.
#include "abi_internal.hpp"

#include <algorithm>
#include <numeric>

using namespace mppi;
using namespace mppi_abi;

namespace {

// the last solve exists and its result can be read: a pending one collected, not lost, not before the first
int last_solve_ready(mppi_handle *h)
{
  int rc = mppi_synchronize(h);
  if (rc) return rc;
  if (h->no_result) return fail(h, MPPI_ERR_HIP, "the last solve timed out: no result");
  if (!h->have_solve) return fail(h, MPPI_ERR_STATE, "no solve yet");
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
  fill_cost_args(h, a.cost);
  if (a.cost.need_control_cost && (step_costs || costs)) {
    // fill_cost_args: a non-zero coefficient, or an exploration_std whose square is not a finite non-zero number
    const bool coeff = h->cost.steering_coeff != 0.0f || h->cost.throttle_coeff != 0.0f;
    return fail(h, MPPI_ERR_UNSUPPORTED,
                coeff ? "a control cost is on: du = eps nu is not recoverable from the applied controls bit for bit (states, controls and "
                        "first_crash are served)"
                      : "exploration_std is zero or not finite, so the control-cost term is not an exact 0, and du = eps nu is not "
                        "recoverable from the applied controls (states, controls and first_crash are served)");
  }
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t S = h->stream;
  if (h->armed) {
    S = h->gstream;
    HIPCHK(h, hipStreamWaitEvent(S, h->ev_arm, 0));
  } else {
    OWN(h);
  }
  const int T = h->T, chunk = h->trace_chunk;
  // the chunk's records in h->d_trace
  float *d_states = h->d_trace;
  float *d_controls = d_states + (size_t)chunk * T * kStateDim;
  float *d_step = d_controls + (size_t)chunk * T * kControlDim;
  float *d_costs = d_step + (size_t)chunk * T;
  int *d_first = reinterpret_cast<int *>(d_costs + chunk);
  for (int i = 0; i < kStateDim; i++) a.state[i] = h->solve_state[i];
  a.V = h->v_buf;
  a.ks = h->d_trace_ks;
  a.wimg = image(h, h->basis ? Image::Theta : Image::Trace);
  a.inv_t = h->d_invt;
  a.states = states ? d_states : nullptr;
  a.controls = controls ? d_controls : nullptr;
  a.step_costs = step_costs ? d_step : nullptr;
  a.costs = costs ? d_costs : nullptr;
  a.first_crash = first_crash ? d_first : nullptr;
  a.K = h->K;
  a.T = T;
  for (int i = 0; i < 2; i++) {
    a.nu[i] = h->cfg.exploration_std[i];
    a.u_lo[i] = h->u_lo[i];
    a.u_hi[i] = h->u_hi[i];
  }
  a.dt = h->dt;
  a.negate_yaw_der = h->cfg.negate_yaw_der ? 1 : 0;
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
  if (!h->have_weights) return fail(h, MPPI_ERR_STATE, "no solve yet (mppi_rollout_only computes no weights)");
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

}  // extern "C"
