/*
 * mppi_hip.h -- C ABI of libmppi_hip.so, the MI355X (gfx950) MPPI solver.
 *
 * Drop-in boundary for the rollout hot path of rdesc/autorally's
 * autorally_control/src/path_integral.  The reference has no FFI for this path:
 * its boundary is the C++ template class MPPIController<DYNAMICS_T, COSTS_T, ...>
 * plus two cnpy-loaded .npz formats.  Each entry point below names the reference
 * interface it replaces; paths are relative to /root/reference/autorally_control/,
 *   PI/ = include/autorally_control/path_integral/.
 *
 * Conventions: extern "C"; opaque handle; every call returns an int status
 * (MPPI_OK == 0); no exceptions cross the ABI; the caller owns every host
 * buffer and the library copies; a handle owns all its device memory and one HIP
 * stream; a handle is single-threaded, distinct handles may be driven from
 * distinct host threads (one per GPU).  On error outputs are left untouched
 * (the reference logs CUDA errors and continues, PI/gpu_err_chk.h:74).
 *
 * There is NO CPU fallback: every compute entry point fails with
 * MPPI_ERR_NO_DEVICE / MPPI_ERR_HIP when no gfx950 device is usable.
 */
#ifndef MPPI_HIP_H_
#define MPPI_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: + mppi_set_costmap_transform, mppi_savitsky_golay, mppi_compute_control_batch[_async], mppi_control_ticks_batch, mppi_nominal_traj_pair,
 *    mppi_debug_inject_handover_fault; mppi_slide_control_seq(h, 0) is MPPI_OK (was MPPI_ERR_INVALID); "fused" =
 *    four-wavefront workgroups; variant names "_fused_b256", "_3w", "_multiN", "_oct8w", "valu_row8w_*"; variants "row", "multi4u". */
/* 3: + mppi_set_host_threads, mppi_compute_feedback_gains_pair. */
/* 4: + mppi_debug_capture_iterations, mppi_debug_get_iterations, mppi_set_wait_timeout, mppi_debug_form_candidates; variants
 *    "row_tree", "row_exact", "row64[_r8|_r16]", "m44"; names "valu_row8w_tree_*", "valu_row64_r*_tree_*", "mfma4x4x1_*_m44_split_tree" (automatic), "mfma4x4x1_*_m44_tree" ("m44_chain"). */
/* 5: solves of more than 4096 rollouts run a one-launch tail (in-launch hand-overs with a deadline: fault roles 32-34 of
 *    mppi_debug_inject_handover_fault); after a wait timeout the lost solve is not waited for again (mppi_set_wait_timeout);
 *    "mfma" / "valu" / "valu_lds" drop a form forced by name; variants "multi1", "multi4u[_gen]", "row64_r8" removed;
 *    + mppi_debug_set_chained_ticks (mppi_control_ticks enqueues one solve ahead), + mppi_debug_min_cost;
 *    + mppi_arm, mppi_arm_batch, mppi_disarm, mppi_is_armed (solve-ahead for a new state every tick; compatible additions). */
/*    (still 5) + rollout variant "lds44", name "mfma4x4x1_lds_l<N>_w<W>": no new export, nothing else changes. */
/*    (still 5) + mppi_debug_launch_info (a debug hook; compatible addition); two handles of the automatic "m44" form or of
 *    "lds44" share a launch in mppi_compute_control_batch / mppi_arm_batch: results unchanged. */
/*    (still 5) + rollout variant "lds128", name "mfma4x4x1_lds2h_l<N>_w<W>": hidden widths up to 128; no new export, nothing
 *    else changes ("lds44" keeps refusing widths above 64). */
/*    (still 5) + mppi_trace_rollouts, mppi_top_rollouts (chosen rollouts of the last solve replayed with their states, clamped
 *    controls and step costs; compatible additions, no kernel form or launch path changes). */
/*    (still 5) + rollout variant "lds16", name "mfma16x16x4_lds_l<N>_w<W>": the throughput form of any layer list up to 128 wide;
 *    no new export.  "valu_lds" reads a parameter blob that does not fit the LDS from global memory instead of failing at its launch. */
/*    (still 5) + rollout variant "bf_row", name "basis_funcs25_row8w": the basis-function model in the row form's group, the bits
 *    of "bf3", by name only; with it the basis-function model has a gated form (mppi_arm, mppi_arm_batch, chained
 *    mppi_control_ticks); no new export, the automatic choice does not change. */
/*    (still 5) + rollout variant "glb16" (and "glb16_r<N>"), name "mfma16x16x4_glb_l<N>_w<W>": "lds16"'s wavefront for every layer list
 *    mppi_create accepts (hidden widths up to 256, an image of any size): the front of the image resident in LDS, the rest read
 *    from global memory; no new export. */
/*    (still 5) + rollout variant "glb44" (and "glb44_r<N>"), name "mfma4x4x1_glb_l<N>_w<W>": "lds128"'s group (the latency form, with
 *    mppi_arm, mppi_arm_batch, chained mppi_control_ticks and the pair in one launch) for every layer list mppi_create accepts
 *    (hidden widths up to 256, an image of any size): the front of the image resident in LDS, the rest read from global memory;
 *    no new export. */
/*    (still 5) + rollout variant "fleet16", name "mfma16x16x4_fleet_l<N>_w<W>": "lds16"'s wavefront, image and lists with the argument
 *    block read from device memory; 2..64 handles forced to it share the launches of mppi_compute_control_batch (one generator, one
 *    rollout, one tail launch per iteration); no new export, no gated form, the automatic choice does not change. */
/*    (still 5) + rollout variant "fleet_multi4", name "mfma16x16x4_h<H>_l<N>_fleet_multi4_tree_gen": the workgroup and the bits of
 *    "multi4_tree_gen" (6-32x2-4, 6-32x4-4, 6-64x2-4) with the argument block read from device memory; 2..64 handles forced to it
 *    share the launches of mppi_compute_control_batch as "fleet16" handles do; no new export, no gated form, the automatic choice
 *    does not change. */
/*    (still 5) + rollout variants "fleet_bf", "fleet_bf_w1", "fleet_bf_w2", "fleet_bf_w3", name "basis_funcs25_fleet[_w<N>]": the
 *    workgroups and the bits of the basis-function model's own kernels with the argument block read from device memory; 2..64
 *    handles forced to it share the launches of mppi_compute_control_batch as "fleet16" handles do; no new export, no gated
 *    form, the automatic choice does not change. */
/*    (still 5) + rollout variant "fleet_glb16" (and "fleet_glb16_r<N>"), name "mfma16x16x4_fleet_glb_l<N>_w<W>": "glb16"'s wavefront,
 *    image and lists with the argument block AND the layer list read from device memory; 2..64 handles forced to it -- of ANY
 *    layer lists and caps -- share the launches of mppi_compute_control_batch as "fleet16" handles do; no new export, no gated
 *    form, the automatic choice does not change. */
/*    (still 5) + rollout variants "row32", "row32_tree", names "valu_row8w_l<N>_w<W>" / "valu_row8w_tree_l<N>_w<W>": the row form
 *    for every layer list of one to four hidden layers up to 32 wide; by name only, gated form and pair launch; no new export, the
 *    automatic choice does not change. */
/*    (still 5) + mppi_compute_feedback_gains_batch, mppi_debug_ddp_info, mppi_debug_device_tanhf (the DDP feedback gains of a fleet
 *    in one launch; compatible additions, the single and the pair call are unchanged). */
/*    (still 5) + mppi_nominal_traj_batch, mppi_debug_nominal_info (the nominal trajectories of a fleet in one launch; compatible
 *    additions, the single and the pair call are unchanged). */
/*    (still 5) + mppi_trace_rollouts_batch, mppi_debug_trace_info (the traces of a fleet in one launch, the largest weights chosen
 *    on the device; compatible additions, mppi_trace_rollouts and mppi_top_rollouts are unchanged). */
/*    (still 5) + mppi_nominal_and_gains_batch, mppi_debug_nominal_and_gains_info (a fleet's nominal trajectories and the feedback
 *    gains that track them in one launch; compatible additions, the two batch calls it equals are unchanged). */
/*    (still 5) + mppi_closed_loop_ticks_batch, mppi_debug_closed_loop_info, mppi_debug_closed_loop_check (closed-loop ticks of a
 *    fleet -- solve, plant step, slide -- enqueued on the device without collecting in between; compatible additions, every call it
 *    equals is unchanged). */
/*    (still 5) + mppi_set_plant_model, mppi_debug_plant_model_info, mppi_plant_drive_batch, mppi_debug_plant_drive_info,
 *    mppi_debug_plant_drive_host, mppi_closed_loop_sim_batch (a plant network of its own per handle, stepped at pose rate under the
 *    reference's interpolated feed-forward and feedback law, for one batched call and inside a closed loop; compatible additions,
 *    mppi_closed_loop_ticks_batch is unchanged). */
#define MPPI_ABI_VERSION 5
#define MPPI_STATE_DIM 7   /* [x, y, yaw, roll, u_x, u_y, yaw_mder]  NeuralNetModel<7,2,3,...> */
#define MPPI_CONTROL_DIM 2 /* [steering, throttle] */
#define MPPI_MAX_LAYERS 8

enum {
  MPPI_OK = 0,
  MPPI_ERR_INVALID = 1,   /* bad argument / size mismatch */
  MPPI_ERR_NO_DEVICE = 2, /* no usable gfx950 device */
  MPPI_ERR_HIP = 3,       /* a HIP runtime call failed; see mppi_last_error */
  MPPI_ERR_STATE = 4,     /* call order (e.g. solve before set_nn_params / set_costmap) */
  MPPI_ERR_UNSUPPORTED = 5
};

typedef struct mppi_handle mppi_handle;

/* Constructor arguments of MPPIController (PI/mppi_controller.cuh:101-102,
 * PI/mppi_controller.cu:321-363) + NeuralNetModel(dt, control_rngs)
 * (PI/neural_net_model.cu:38-67) + the template constants of
 * src/path_integral/path_integral_main.cu:65-78 made runtime values. */
typedef struct {
  int device;                 /* HIP device ordinal */
  int num_rollouts;           /* K; must be a multiple of 64 (mppi_controller.cuh:58-60) */
  int num_timesteps;          /* T */
  int hz;                     /* dt = (float)(1.0/hz) */
  int optimization_stride;    /* opt_delay of rolloutKernel */
  float gamma;
  int num_iters;
  int n_layers;               /* entries of layers[], input and output included; 0 selects the reference's
                               * other dynamics family, GeneralizedLinear<CarBasisFuncs,7,2,25,CarKinematics,3>
                               * (path_integral_main.cu:70-74): parameters by mppi_set_bf_params */
  int layers[MPPI_MAX_LAYERS];/* e.g. {6,32,32,4}; layers[0]==6, layers[n-1]==4 */
  float exploration_std[2];   /* nu */
  float init_control[2];      /* init_u */
  float control_min[2];       /* control_rngs_[i].x */
  float control_max[2];       /* control_rngs_[i].y */
  int negate_yaw_der;
  uint64_t seed;              /* reference: 1234 (mppi_controller.cu:331) */
} mppi_config;

/* MPPICosts::CostParams scalars (PI/costs.cuh:67-85) + l1_cost_ (costs.cuh:276).
 * The transform (r_c1, r_c2, trs) travels with the costmap, see mppi_set_costmap. */
typedef struct {
  float desired_speed;
  float speed_coeff;
  float track_coeff;
  float max_slip_ang;
  float slip_penalty;
  float track_slop;
  float crash_coeff;
  float steering_coeff;
  float throttle_coeff;
  float boundary_threshold;
  float discount;
  int l1_cost;
} mppi_cost_params;

/* Per-stage device times of the most recent solves (HIP events on the handle's stream). */
typedef struct {
  int n_solves;            /* solves accumulated since mppi_reset_stage_times */
  float noise_ms;          /* sums over n_solves */
  float rollout_ms;
  float weights_ms;
  float reduction_ms;      /* weighted reduction + Savitzky-Golay */
  float total_ms;          /* first launch -> last kernel end */
} mppi_stage_times;

int mppi_abi_version(void);
const char *mppi_strerror(int status);
/* Last HIP/validation error text of this handle ("" if none). */
const char *mppi_last_error(const mppi_handle *h);
/* Number of visible HIP devices whose architecture is gfx950 (0 if none / no runtime). */
int mppi_device_count(void);

/* MPPIController::MPPIController + allocateCudaMem (mppi_controller.cu:321-387). */
int mppi_create(const mppi_config *cfg, mppi_handle **out);
/* deallocateCudaMem (mppi_controller.cu:389-400), without the double free of Q14. */
int mppi_destroy(mppi_handle *h);

/* GeneralizedLinear::setParams / loadParams / paramsToDevice (PI/generalized_linear.cu:86-118):
 * W row-major [4][25] (the .npz key "W"), n == 100.  Only for handles created with n_layers == 0.
 * The basis functions are CarBasisFuncs (PI/car_bfs.cuh:44-120); the yaw rate is always negated
 * (generalized_linear.cu:216), negate_yaw_der is ignored. */
int mppi_set_bf_params(mppi_handle *h, const float *W, size_t n);
/* NeuralNetModel::paramsToDevice (neural_net_model.cu:120-150): theta is the packed
 * [W1|b1|W2|b2|...] blob, n == NUM_PARAMS. The .npz is read by the C++ host layer. */
int mppi_set_nn_params(mppi_handle *h, const float *theta, size_t n);
/* NeuralNetModel::updateModel (neural_net_model.cu:152-180): data = [W1|W2|..|b1|b2|..]. */
int mppi_update_model(mppi_handle *h, const int *description, int n_desc, const float *data, size_t n);
/* control_rngs_ (cutThrottle, mppi_controller.cu:460-466, sets control_max[1]=0). */
int mppi_set_control_limits(mppi_handle *h, const float umin[2], const float umax[2]);

/* MPPICosts::loadTrackData/updateTransform/costmapToTexture (costs.cu:190-232, 175-188,
 * 128-154): rgba = float4[H][W] (x fastest).  Texture semantics reproduced: point
 * filter, clamp, normalised coordinates. */
int mppi_set_costmap(mppi_handle *h, int width, int height, const float *rgba,
                     const float r_c1[3], const float r_c2[3], const float trs[3]);
/* MPPICosts::updateTransform + paramsToDevice (costs.cu:175-188, 234-238): the coordinate transform alone
 * (r_c1, r_c2, trs are public members of CostParams; the texture stays). */
int mppi_set_costmap_transform(mppi_handle *h, const float r_c1[3], const float r_c2[3], const float trs[3]);
/* costmapToTexture(float*, channel) (costs.cu:101-126). */
int mppi_set_costmap_channel(mppi_handle *h, int channel, const float *data, size_t n);
/* updateParams / updateParams_dcfg / paramsToDevice (costs.cu:156-173, 75-87, 234-238). */
int mppi_set_cost_params(mppi_handle *h, const mppi_cost_params *p);

/* U_ accessors (resetControls :448-458; setControlSequence-like). U is [T][2]. */
int mppi_reset_controls(mppi_handle *h);
int mppi_set_control_seq(mppi_handle *h, const float *U, size_t n);
int mppi_get_control_seq(mppi_handle *h, float *U, size_t n);
/* control_hist_ (mppi_controller.cu:347, 528-541): two controls executed before U_0. */
int mppi_set_control_hist(mppi_handle *h, const float hist[4]);
int mppi_get_control_hist(mppi_handle *h, float hist[4]);
/* savitskyGolay() (mppi_controller.cuh:134, mppi_controller.cu:468-499) as a call of its own: smooths the
 * handle's current U_ in place with control_hist_ as left padding (computeControl already ends with it). */
int mppi_savitsky_golay(mppi_handle *h);
/* slideControlSeq (mppi_controller.cu:527-554), flat-index quirk for stride>2 kept. */
int mppi_slide_control_seq(mppi_handle *h, int stride);

/* Replaces curandCreateGenerator/SetSeed (mppi_controller.cu:330-331): this build's
 * MRG32k3a generator, one 2^76-draw subsequence per rollout, `offset` draws skipped. */
int mppi_seed(mppi_handle *h, uint64_t seed, uint64_t offset);
/* Explicit-noise mode (what the parity tests use): eps = [num_iters][K][T][2] N(0,1),
 * consumed by the NEXT mppi_compute_control / mppi_rollout_only instead of the generator. */
int mppi_set_noise(mppi_handle *h, const float *eps, size_t n);
/* Runs the generator for one iteration worth of draws ([K][T][2]) and copies it out;
 * advances the stream exactly as a solve iteration would. */
int mppi_generate_noise(mppi_handle *h, float *eps_out, size_t n);

/* MPPIController::computeControl(state) up to and including savitskyGolay()
 * (mppi_controller.cu:600-671); computeNominalTraj is mppi_nominal_traj. Blocking. */
int mppi_compute_control(mppi_handle *h, const float state[MPPI_STATE_DIM]);
/* n_ticks times { mppi_compute_control(state); mppi_slide_control_seq(stride) } without returning to the
 * caller in between: the body of runControlLoop's tick for one controller (run_control_loop.cuh:207-219)
 * for callers -- bench.py -- whose own per-call overhead (an interpreter, an FFI) would otherwise sit
 * inside the solve-to-solve time.  stride = 0 skips the slide.  Stops at the first error. */
int mppi_control_ticks(mppi_handle *h, const float state[MPPI_STATE_DIM], int n_ticks, int stride);
/* Same solve, enqueued only; results are valid after mppi_synchronize. */
int mppi_compute_control_async(mppi_handle *h, const float state[MPPI_STATE_DIM]);
int mppi_synchronize(mppi_handle *h);
/* The solves of n independent controllers enqueued together -- runControlLoop's tick
 * (PI/run_control_loop.cuh:218-219: actual-state and predicted-state controller, both of path_integral_main.cu:119-122)
 * -- states is [n][7], handles[i] solves from states + 7 i.  Where the handles' rollout kernels can share a launch
 * (network model, same layer list and num_iters, all groups of 16 rollouts together at most one per CU: 2 x K=1920 on
 * 256 CUs; the forms that have a batched kernel: the four-wavefront form and the row forms for n <= 4, the automatic
 * "m44" form of 64-wide nets and "lds44" / "lds128" / "glb44" / "row32" / "row32_tree" -- forced on every handle, the whole layer list (and "glb44"'s cap) equal -- for n == 2; the
 * basis-function model's three-wavefront form, or its "bf_row" form forced on both handles of a pair under the row forms' rule:
 * 2 x K=1920 shares a launch, 2 x K=2560 does not) the n solves cost TWO kernel launches in all, on a stream of the library
 * shared by the device's handles; otherwise ("m44_chain", three m44 handles ...) this is n calls of
 * mppi_compute_control_async.
 * The "fleet16" variant: 2 <= n <= 64 handles share their launches when every handle is forced to "fleet16", all are on one device,
 * have the same whole layer list, the same num_iters and the same pair (affine costmap transform, control cost needed), K <= 4096
 * each, none has stage timing, capture or prefetched draws, and every handle is ready.  Each iteration of such a batch is THREE
 * launches in all on the library's stream of the device -- one generator launch, one rollout launch, one tail launch -- whatever
 * else differs between the instances (K, T, state, U and hist, weights, costmap and transform, cost parameters, limits, nu,
 * gamma, seed, explicit noise or the generator).  Any other set of such handles (n > 64, a mixed set, a K above 4096) is n
 * per-handle solves; a set of "fleet16" handles with one that is not ready returns that handle's error before any has moved.
 * The "fleet_multi4" variant: the same rule and the same three launches for 2 <= n <= 64 handles that are ALL forced to
 * "fleet_multi4" (one of 6-32x2-4, 6-32x4-4, 6-64x2-4); a set that mixes "fleet16" and "fleet_multi4" handles is n per-handle solves.
 * The "fleet_bf" variant (the basis-function model): the same rule and the same three launches for 2 <= n <= 64 handles that are
 * ALL forced to "fleet_bf", or all to the same "fleet_bf_w<N>"; the layer list plays no part, the forced wave count must agree.
 * The "fleet_glb16" variant: the same three launches for 2 <= n <= 64 handles that are ALL forced to "fleet_glb16" (with or without
 * "_r<N>"); the handles' layer lists and caps need NOT agree -- every instance of the launch brings its own -- and everything else
 * of the rule stands (one device, one num_iters, one pair of cost flags, K <= 4096 each, no timing, capture, prefetched draws or
 * armed handle, all ready); a set that mixes it with any other form is n per-handle solves.
 * mppi_debug_launch_info tells which it was.  Either way every
 * handle's results are bit for bit those of its own mppi_compute_control, collected per handle with
 * mppi_synchronize / mppi_get_results.  The blocking form waits for all of them. */
int mppi_compute_control_batch_async(mppi_handle *const *handles, const float *states, int n);
int mppi_compute_control_batch(mppi_handle *const *handles, const float *states, int n);
/* Solve-ahead: the launch call and the dispatch of the NEXT solve leave the control step.  mppi_arm enqueues this handle's next
 * solve now, gated: its kernels start (weights, first noise) and wait at most max_wait_s (0 < max_wait_s <= 0.1) for the next
 * mppi_compute_control[_async] to supply the state -- that call does not launch, it writes its state, the host's U and hist into
 * the gate and opens it.  May be called with a solve pending (the armed one goes behind it) or idle.  MPPI_ERR_UNSUPPORTED
 * (nothing enqueued, handle unchanged) where the handle's form / configuration has no gated form: num_iters > 1, the
 * basis-function model in any form but "bf_row", forms other than the row forms, the automatic m44 form, "lds44", "lds128", "glb44", "row32", "row32_tree", "bf_row"
 * and the automatic multi4-tree form with its generator kernel, stage timing, capture, explicit noise.  Results are bit for bit those of the same calls without mppi_arm;
 * the slide stride between ticks may vary, and mppi_set_control_seq / _hist between arm and compute go through the gate.
 * Every call that changes what the armed solve would compute (model, cost, costmap, limits, seed, noise, variant, timing,
 * capture, mppi_rollout_only, mppi_control_ticks, the debug entries, mppi_destroy) calls it off first; the generator stream is
 * then where it would be had the handle never been armed.  mppi_get_results and mppi_get_applied_controls are served without
 * waiting on the armed kernels.  A compute that arrives after max_wait_s (a margin inside it) calls the armed solve off and
 * solves unarmed, with the same bits.  The device's batch stream is shared: a batch of other handles enqueued while a batch is
 * armed runs after that batch's gate opens. */
int mppi_arm(mppi_handle *h, double max_wait_s);
/* The same for the solves of one mppi_compute_control_batch[_async](handles, states, n) call: the shared one-launch form where
 * the batch would use it and the form has a gated batched kernel (the row forms; two handles of the automatic "m44" form or of
 * "lds44" or of "lds128" or of "glb44" or of "row32" / "row32_tree" or of "bf_row"), otherwise each handle armed on its own where it can be
 * (MPPI_ERR_UNSUPPORTED if one could not be; the others stay armed).  Only a batch call with the same handles in the same order
 * opens the gates; any other call on one of them calls the whole armed launch off first. */
int mppi_arm_batch(mppi_handle *const *handles, int n, double max_wait_s);
/* Calls the armed solve off (its gate opens with the cancel bit); never blocks on the GPU. */
int mppi_disarm(mppi_handle *h);
/* 1 while a solve is armed, else 0. */
int mppi_is_armed(const mppi_handle *h);
/* mppi_control_ticks for several controllers: n_ticks times { mppi_compute_control_batch; mppi_slide_control_seq
 * (handles[i], stride) for every i } -- the solve part of runControlLoop's tick for its two controllers. */
int mppi_control_ticks_batch(mppi_handle *const *handles, const float *states, int n, int n_ticks, int stride);
/* getComputedTrajectoryCost (:683-687) + optional per-rollout vectors of the last
 * iteration: costs[K] (traj_costs_ after the rollout), weights[K] (after normExpKernel). */
int mppi_get_results(mppi_handle *h, float *U, float *traj_cost, float *costs, float *weights);
/* The rewritten du_d buffer of the last iteration, [K][T][2] (applied, unclamped controls, Q3). */
int mppi_get_applied_controls(mppi_handle *h, float *V, size_t n);
/* The rollouts ks[0..n) of the most recent completed solve (last iteration), replayed on the device from that solve's
 * vehicle state and its applied controls (the buffer mppi_get_applied_controls reads), with the handle's current model, cost
 * parameters, costmap and control limits.  Any output may be NULL.
 *   states      [n][T][7]  state BEFORE the update of step t (states[i][0] = the solve's state): what the cost of step t saw
 *   controls    [n][T][2]  the controls after the clamp (what the dynamics saw)
 *   step_costs  [n][T]     computeCost of step t (0 at t = 0, which is never costed, Q5)
 *   costs       [n]        the running mean the rollout kernel stores in traj_costs_
 *   first_crash [n]        the first step whose cost saw the crash flag set, -1: never
 * Every neuron is summed in the reference's order: costs[i] is costs[ks[i]] of mppi_get_results bit for bit on every rollout
 * form that keeps that order in every layer (not the forms that sum a layer as a butterfly -- "row_tree", "m44", "m44_chain",
 * "multi4_tree", "row64" --, whose costs differ by their re-association only).  Valid wherever mppi_get_applied_controls is:
 * a pending solve is waited for first; MPPI_ERR_HIP after a lost solve; mppi_slide_control_seq / mppi_set_control_seq
 * afterwards change nothing it returns.  While armed the handle stays armed and the trace is enqueued on the generator stream
 * in FRONT of the armed kernels, not behind them -- but its workgroups (four wavefronts of 160 / 192 VGPRs, up to 64 KB of LDS)
 * still need room on the chip beside the gated kernels, which hold theirs until the gate opens: there is room on every CU
 * beside an armed row launch; an armed "m44" / "lds44" / "lds128" / "glb44" launch fills the SIMDs of the CUs it occupies, and the trace
 * runs on the CUs it left free (16 of 256 for the pair of K = 1920).  Where an armed launch occupies every CU the trace ends
 * only once the gate opens or max_wait_s runs out: trace before arming there.
 * Duplicate indices are allowed, n == 0 does nothing.  MPPI_ERR_STATE before the first solve (mppi_rollout_only counts: its
 * state, controls and costs are what is traced) and after a solve whose launch failed; MPPI_ERR_INVALID for ks == NULL with
 * n > 0, n < 0, an index outside [0, K).  With a control cost on (steering_coeff or throttle_coeff non-zero, or an
 * exploration_std whose square is zero or not finite) du = eps nu cannot be had back from the applied controls bit for bit:
 * step_costs != NULL or costs != NULL is then MPPI_ERR_UNSUPPORTED (reason in mppi_last_error); states, controls and
 * first_crash are served.  (csrc/rollout_trace.hip: one wavefront per rollout, one lane per neuron.) */
int mppi_trace_rollouts(mppi_handle *h, const int *ks, int n, float *states, float *controls,
                        float *step_costs, float *costs, int *first_crash);
/* ks[0..n) = indices of the n largest weights of the last solve, descending, ties to the lower index (host work);
 * MPPI_ERR_INVALID for n < 0 or n > K or ks == NULL with n > 0, MPPI_ERR_STATE before the first solve (mppi_rollout_only
 * computes no weights: it does not count). */
int mppi_top_rollouts(mppi_handle *h, int n, int *ks);
/* The traces of a whole fleet in one call: handle i traces counts[i] rollouts of its last solve -- the indices ks[i][0..counts[i]),
 * or, where ks is NULL as a whole or ks[i] is NULL, its counts[i] largest weights in mppi_top_rollouts' order.  ks_out (NULL, or
 * [n_handles]): ks_out[i] receives the counts[i] indices that were traced.  states, controls, step_costs, costs, first_crash: each
 * NULL as a whole (not wanted) or [n_handles] pointers to buffers of mppi_trace_rollouts' shapes for counts[i] rollouts; where an
 * array is given, the entry of every handle with counts[i] > 0 must be non-NULL.  Per handle the result is that of
 * mppi_top_rollouts (where it chooses) followed by mppi_trace_rollouts: the last completed solve, its state and applied controls,
 * the current model, cost, costmap and limits, duplicates allowed.
 * Sharing rule: n_handles >= 2, all on one device, none armed, every counts[i] <= min(K_i, 1024): the set is traced ON THE DEVICE'S
 * BATCH STREAM -- the largest weights are chosen on the device from K alone (no weight travels to the host; any K), the network
 * handles share one launch per 64 (layer lists, K, T, scene and limits are data), the basis-function handles one of their own;
 * one copy of the explicit indices in, ONE copy of the outputs that were asked for out, one synchronise.  Every record is bit for
 * bit the per-handle call's.  Anything else -- n_handles = 1, an armed handle in the set (handles armed together wait gated on the
 * batch stream; the per-handle call goes in front of its own gate, and the handle stays armed), a count above 1024, several
 * devices -- runs the per-handle calls one after the other, with their bits; mppi_debug_trace_info tells which it was.
 * Order of work: every argument is checked -- MPPI_ERR_INVALID for NULL handles or counts, n_handles < 1, a NULL handle, a handle
 * listed twice, a negative count, a count above K where the handle chooses, an index outside [0, K), a missing output pointer --,
 * then every pending solve is collected, then every handle's readiness (MPPI_ERR_STATE before the first solve, and for a choice of
 * the largest weights after mppi_rollout_only alone; MPPI_ERR_HIP after a lost solve) and the control-cost rule (MPPI_ERR_UNSUPPORTED
 * if step_costs or costs is given and ANY handle with rollouts to trace has a control cost on; the reason is in that handle's
 * mppi_last_error; the same call without the two cost arrays is served); only then is anything launched.  On the shared path the
 * caller's buffers are written after EVERY launch and copy of the call has succeeded.  All counts 0: MPPI_OK, nothing is written.
 * The call blocks until the results are back.  (csrc/rollout_trace.hip, csrc/abi_trace.hip.) */
int mppi_trace_rollouts_batch(mppi_handle *const *handles, int n_handles, const int *counts, const int *const *ks, int *const *ks_out,
                              float *const *states, float *const *controls, float *const *step_costs, float *const *costs,
                              int *const *first_crash);
/* Test / tooling hook: *on_device = 1 if the handle's most recent trace ran in the fleet's kernels (the shared path of
 * mppi_trace_rollouts_batch), 0 if in a launch of its own (or none yet).  MPPI_ERR_INVALID for a NULL argument. */
int mppi_debug_trace_info(const mppi_handle *h, int *on_device);
/* Stage-level entry: noise (or explicit noise) + rolloutKernel only; costs[K]. */
int mppi_rollout_only(mppi_handle *h, const float state[MPPI_STATE_DIM], float *costs);
/* computeNominalTraj (mppi_controller.cu:501-519), host replay of U_ like the reference:
 * state_seq [T][7], control_seq [T][2] (clamped). */
int mppi_nominal_traj(mppi_handle *h, const float state[MPPI_STATE_DIM], float *state_seq,
                      float *control_seq);

/* computeNominalTraj of the two controllers of a control tick (run_control_loop.cuh:218-219: both end their
 * computeControl with it) in one call: two network replays of the same length advance in lockstep on the host, at about the
 * cost of one; results bit for bit those of two mppi_nominal_traj calls (which is what this does for any other pair). */
int mppi_nominal_traj_pair(mppi_handle *ha, const float state_a[MPPI_STATE_DIM], float *state_seq_a, float *control_seq_a,
                           mppi_handle *hb, const float state_b[MPPI_STATE_DIM], float *state_seq_b, float *control_seq_b);

/* computeNominalTraj of a whole fleet in one call: handles[n], states [n][7]; handle i's replay of its current control sequence
 * lands in state_seqs[i] ([T_i][7]) and control_seqs[i] ([T_i][2], clamped).
 * Sharing rule: n >= 2 handles of the network model with parameters set, all on one device, are replayed ON THE DEVICE, one
 * workgroup per controller in one launch (nominal_fleet_kernel; more than 64 handles: launches of up to 64) -- layer lists, T,
 * hz, limits and negate_yaw_der may differ per handle.  The kernel restates mppi_nominal_traj statement for statement (the clamp's
 * two branches, every fmaf, the bias add, libm's tanhf bits, the Euler step); only sinf / cosf of the heading are the rounded
 * double results, not glibc's floats (1 ulp apart in 1.3 % of headings): control_seq is bit for bit the single call's, state_seq
 * agrees far inside the bound both are held to, and bit for bit while the heading stays 0.  Anything else -- n = 1, a
 * basis-function handle in the set, handles on several devices -- runs n mppi_nominal_traj calls on the host with their bits;
 * mppi_debug_nominal_info tells which it was.
 * Order of work: every argument is checked (MPPI_ERR_INVALID for a NULL array, n < 1, a NULL handle or output pointer in the set,
 * a handle listed twice), then every handle's readiness (MPPI_ERR_STATE without parameters), then every pending solve is collected
 * (as mppi_nominal_traj does); only then is an output written or anything launched.  The caller's buffers are written after EVERY
 * launch of the call has succeeded: MPPI_ERR_HIP from any of them leaves all of them as they were.  The inputs are each handle's
 * HOST control sequence and the call's state.  The call uses the device's batch stream and blocks until the results are back; it touches no
 * handle's solve state beyond collecting pending solves, and an armed handle stays armed -- but handles armed TOGETHER
 * (mppi_arm_batch) wait gated on the batch stream, and this call's launch waits behind their gate: replay before arming, or after
 * the gate has opened. */
int mppi_nominal_traj_batch(mppi_handle *const *handles, const float *states /* n x 7 */, float *const *state_seqs /* [i]: T_i x 7 */,
                            float *const *control_seqs /* [i]: T_i x 2 */, int n);
/* Test / tooling hook: *on_device = 1 if the handle's most recent nominal replay ran in the fleet's kernel, 0 if on the host (or
 * none yet).  MPPI_ERR_INVALID for a NULL argument. */
int mppi_debug_nominal_info(const mppi_handle *h, int *on_device);

/* computeFeedbackGains (PI/mppi_controller.cu:431-441) -> DDP::run (ddp/ddp.h:49-157), one
 * iteration, dt = 1/hz, from `state`, tracking target_state_seq [T][7] / target_control_seq [T][2]
 * -- the reference passes state_solution_ / control_solution_ of the last computeControl, which for
 * the predicted-state controller were NOT computed from `state` (run_control_loop.cuh:218-225).
 * Both NULL: the nominal trajectory of the current control sequence from `state`.
 * Host computation like the reference (T Jacobians of the network via computeGrad,
 * neural_net_model.cu:233-264, and T-1 sequential 7x7 Riccati steps).  Weights default to initDDP's
 * Q = diag(.5,.5,.25,0,.05,.01,.01), R = diag(10,10), Qf = 0 (mppi_controller.cu:410-417).
 * Returns MPPI_ERR_STATE where the reference exits (-3) on a failed LDLT. */
int mppi_set_ddp_weights(mppi_handle *h, const float Q[MPPI_STATE_DIM], const float R[MPPI_CONTROL_DIM],
                         const float Qf[MPPI_STATE_DIM]);
int mppi_compute_feedback_gains(mppi_handle *h, const float state[MPPI_STATE_DIM],
                                const float *target_state_seq, const float *target_control_seq);
/* getFeedbackGains (:443-446), OptimizerResult (ddp/result.h): feedback [T][2][7] (the last one is
 * zero), feedforward [T][2], state_traj [T][7], control_traj [T][2], total_cost; any may be NULL. */
int mppi_get_feedback_gains(mppi_handle *h, float *feedback, float *feedforward, float *state_traj,
                            float *control_traj, float *total_cost);

/* computeFeedbackGains of the two controllers of a control tick (run_control_loop.cuh:220-225: both, one after the other, on
 * the optimizer thread) in one call; results bit for bit those of two mppi_compute_feedback_gains calls.  With
 * mppi_set_host_threads(2) the two DDP passes run side by side. */
int mppi_compute_feedback_gains_pair(mppi_handle *ha, const float state_a[MPPI_STATE_DIM], const float *target_state_seq_a,
                                     const float *target_control_seq_a, mppi_handle *hb, const float state_b[MPPI_STATE_DIM],
                                     const float *target_state_seq_b, const float *target_control_seq_b);

/* computeFeedbackGains of a whole fleet in one call: handles[n], states [n][7], the targets of handle i at
 * target_state_seqs[i] / target_control_seqs[i].  Either array may be NULL as a whole, and entry i of both may be NULL together:
 * that handle tracks its nominal trajectory from the host replay, as in the single call.  Results land in every handle as after
 * its own mppi_compute_feedback_gains (mppi_get_feedback_gains is unchanged).
 * Sharing rule: n >= 2 handles of the network model with parameters set, all on one device, run ON THE DEVICE, one workgroup per
 * controller in one launch (ddp_fleet_kernel; more than 64 handles: launches of up to 64) -- layer lists, T, hz, limits and
 * weights may differ per handle.  The kernel restates the host pass operation for operation (its tanhf returns libm's bits); only
 * sinf / cosf of the heading are the rounded double results, not glibc's floats (1 ulp apart in 1.3 % of headings), so the gains
 * agree with the single call's far inside the bound both are held to, not bit for bit.  Anything else -- n = 1, a basis-function
 * handle in the set, handles on several devices, a handle without parameters -- runs n host passes with the bits (and errors) of n
 * single calls; mppi_debug_ddp_info tells which it was.
 * A handle whose factorisation fails has no result (mppi_get_feedback_gains fails) and its own mppi_last_error; the call then
 * returns MPPI_ERR_STATE and every other handle keeps a valid result.  The call uses the device's batch stream and blocks until
 * the results are back; it touches no handle's solve state (with targets given a pending or armed solve of the same handles is
 * untouched; without, the nominal replay collects the handle's pending solve as the single call does). */
int mppi_compute_feedback_gains_batch(mppi_handle *const *handles, const float *states, const float *const *target_state_seqs,
                                      const float *const *target_control_seqs, int n);
/* Test / tooling hook: *on_device = 1 if the handle's most recent DDP pass ran in the fleet's kernel, 0 if on the host (or none
 * yet).  MPPI_ERR_INVALID for a NULL argument. */
int mppi_debug_ddp_info(const mppi_handle *h, int *on_device);
/* Test hook: out[i] = the DDP kernel's tanhf of in[i], computed on `device` (n floats; the text of csrc/tanhf_scalar.hpp, which has
 * to return the C library's bits).  MPPI_ERR_INVALID for a NULL pointer, n = 0 or a negative device. */
int mppi_debug_device_tanhf(int device, const float *in, float *out, size_t n);

/* The two closing stages of a fleet's tick in one call -- computeNominalTraj, then computeFeedbackGains(state) from the same state
 * (what the reference's tick does after every computeControl): handles[n], states [n][7].  Per handle the result is that of
 * mppi_nominal_traj_batch followed by mppi_compute_feedback_gains_batch with that call's outputs as targets: the nominal sequences
 * land in state_seqs[i] ([T_i][7]) and control_seqs[i] ([T_i][2], clamped), the gains in the handle (mppi_get_feedback_gains is
 * unchanged).  The inputs are each handle's HOST control sequence and the call's state.
 * Sharing rule: where BOTH calls would share a launch -- n >= 2 handles of the network model with parameters set, all on one
 * device -- the two stages are ONE launch (nominal_gains_fleet_kernel, one workgroup per controller; more than 64 handles: launches of
 * up to 64 with one input copy, one result copy and one synchronise per call): the replay runs on one wave while another runs the
 * DDP pass's initial rollout, and the targets never travel through the host.  Layer lists, T, hz, limits, negate_yaw_der and DDP
 * weights may differ per handle.  The results are BIT FOR BIT those of mppi_nominal_traj_batch followed by
 * mppi_compute_feedback_gains_batch(handles, states, state_seqs, control_seqs, n).  The gains therefore track the DEVICE replay,
 * which differs from the host replay that mppi_compute_feedback_gains_batch(..., NULL, NULL, ...) tracks only through sinf / cosf
 * of the heading (the rounded double results, not glibc's floats).  Anything else -- n = 1, a basis-function handle in the set,
 * handles on several devices, a handle without parameters -- runs exactly those two calls one after the other, with their bits and
 * their errors; mppi_debug_nominal_and_gains_info tells which it was.  Below the crossovers of DESIGN 4.20 / 4.21 (a few handles)
 * the host calls (mppi_nominal_traj, mppi_compute_feedback_gains) serve a caller better than any of the batched ones.
 * Order of work, as in mppi_nominal_traj_batch: every argument is checked (MPPI_ERR_INVALID for a NULL array, n < 1, a NULL handle
 * or output pointer in the set, a handle listed twice), then every handle's readiness, then every pending solve is collected; only
 * then is anything launched.  The caller's buffers and every handle's DDP result are written only after every launch and copy
 * of the call has succeeded.  A handle whose factorisation fails has no gains and its own mppi_last_error; its nominal sequences
 * are still delivered, the call returns MPPI_ERR_STATE and every other handle keeps a valid result.  The call uses the device's
 * batch stream and blocks until the results are back; it touches no handle's solve state beyond collecting pending solves, and an
 * armed handle stays armed (handles armed TOGETHER: see mppi_nominal_traj_batch). */
int mppi_nominal_and_gains_batch(mppi_handle *const *handles, const float *states /* n x 7 */,
                                 float *const *state_seqs /* [i]: T_i x 7 */, float *const *control_seqs /* [i]: T_i x 2 */, int n);
/* Test / tooling hook: *fused = 1 if the handle's most recent mppi_nominal_and_gains_batch ran in the one kernel, 0 if as the two
 * calls (or none yet).  MPPI_ERR_INVALID for a NULL argument. */
int mppi_debug_nominal_and_gains_info(const mppi_handle *h, int *fused);

/* Closed-loop ticks of a whole fleet in one call: handles[n]; states [n][7] holds every controller's start state and receives its
 * final one.  The plant is the handle's own dynamics model.  The call is EXACTLY this loop of public calls, which is its reference:
 *     for tick in 0 .. n_ticks-1:
 *         mppi_compute_control_batch(handles, s, n)
 *         mppi_nominal_traj_batch(handles, s, state_seqs, control_seqs, n)
 *         log s_i, control_seqs_i[0 .. stride), the trajectory cost of handle i
 *         s_i = state_seqs_i[stride]
 *         mppi_slide_control_seq(handle_i, stride)
 * with 1 <= stride < min T_i.  The logs are optional (each array, and each entry, may be NULL): state_log[i] receives
 * [n_ticks + 1][7] (row 0 the start state, row t + 1 the state after tick t), control_log[i] [n_ticks][stride][2] (the clamped
 * controls the plant applied), cost_log[i] the n_ticks trajectory costs.  Afterwards every handle is bit for bit where the loop
 * leaves it: the host's U and history, mppi_get_results and mppi_get_applied_controls of the last tick, the generator stream, the
 * device copy of U (the next solve uploads nothing).
 * Device path: 2..64 handles that share the launches of mppi_compute_control_batch (all forced to "fleet16", all to
 * "fleet_multi4" or all to "fleet_glb16") AND the launch of mppi_nominal_traj_batch, with num_iters == 1 and no explicit noise,
 * stage timing or capture: all n_ticks are enqueued on the device's batch stream and the host waits for none of them -- per tick
 * the argument copy, the plant step of the tick before (plant_fleet_kernel: the first `stride` steps of nominal_fleet_kernel's
 * replay, its bits, from a state that stays on the device), the generator, the rollout and the tail, which smooths and slides the
 * device copy of U.  Only the ring of four staging slots of the argument block holds the host back.  The last tick is collected
 * as any solve is; the host's U / history are then read back from the device copy and the logs arrive in one copy.
 * mppi_set_wait_timeout applies to every tick of progress (the sequence number in the result block), not to the whole run.
 * Fallback: every other set -- n = 1, more than 64 handles, a basis-function handle, mixed or latency forms, num_iters > 1,
 * explicit noise, several devices, timing or capture -- runs the loop above literally, with its bits; such a set takes the host's
 * sinf / cosf in the plant wherever mppi_nominal_traj_batch replays on the host.  mppi_debug_closed_loop_info tells which it was.
 * Order of work, as in mppi_nominal_traj_batch: every argument is checked (MPPI_ERR_INVALID: a NULL array or handle, n < 1,
 * n_ticks < 1, a handle listed twice, stride outside [1, min T_i)), then every handle's readiness (MPPI_ERR_STATE), then pending
 * solves of the set are collected and its armed handles disarmed; only then does anything move.
 * Failure (device path): the ticks run on behind a bad one, so the host checks after the run.  A tick whose eta is below 1 or not
 * finite, or whose applied controls are not finite, makes the call return MPPI_ERR_HIP; mppi_last_error of handles[0] and of the
 * handle names the tick and the handle.  EVERY handle of the set is then distrusted: the host's U / history are what they were
 * before the call, the next solve uploads them again, `states` is unchanged, the logs hold the ticks before the failure
 * (mppi_debug_closed_loop_info counts them), the result getters refuse until a solve completes, and the generator streams are where
 * the run left them.  A run longer than 1024 ticks is enqueued and collected in pieces of 1024 (a failure in a later piece still
 * puts U, history and `states` back to what they were before the CALL); the staging ring's wait inside a piece is not bounded by
 * mppi_set_wait_timeout.
 * Other threads: the device's fleet argument block is held only while a piece is being enqueued, not through its waits -- batched
 * solves, replays and DDP passes of other handles on the device queue behind the run on the batch stream; a second closed-loop call
 * on the device waits for the first.
 * Tools only: the environment variable MPPI_CLOSED_LOOP_DEVICE=0, read at every call, sends every set through the loop of public
 * calls (tools/fleet_time.py --closed-loop times the two against each other in one process); not meant for applications. */
int mppi_closed_loop_ticks_batch(mppi_handle *const *handles, float *states /* n x 7, in: start, out: final */, int n, int n_ticks,
                                 int stride, float *const *state_log /* [i]: (n_ticks+1) x 7, or NULL */,
                                 float *const *control_log /* [i]: n_ticks x stride x 2 (clamped, applied), or NULL */,
                                 float *const *cost_log /* [i]: n_ticks trajectory costs, or NULL */);
/* Test / tooling hook: *on_device = 1 if the handle's most recent mppi_closed_loop_ticks_batch ran the device path, 0 if the loop of
 * public calls (or none yet); *ticks = the ticks that call completed.  MPPI_ERR_INVALID for a NULL argument. */
int mppi_debug_closed_loop_info(const mppi_handle *h, int *on_device, int *ticks);
/* Test hook: the host's check behind a device run over one handle's logs -- etas [n_ticks], controls [n_ticks][stride][2]:
 * *bad_tick = the first tick whose eta is below 1 or not finite or whose controls are not finite, -1 if there is none.  No device
 * is needed.  MPPI_ERR_INVALID for a NULL argument, n_ticks < 1 or stride < 1. */
int mppi_debug_closed_loop_check(const float *etas, const float *controls, int n_ticks, int stride, int *bad_tick);

/* A plant of its own.  mppi_closed_loop_ticks_batch steps the controller's own network once per control period, open loop: the
 * reference's debug_mode self-simulation.  The entries below give every handle a plant that is a DIFFERENT network, stepped
 * `substeps` times per control period (pose rate), and driven by the reference's interpolated feed-forward and feedback law
 * (AutorallyPlant::pubControl, autorally_plant.cpp:217-253; SimPlant::controlAt of host/run_control_loop.hpp).
 *
 * mppi_set_plant_model: the plant's network -- any layer list mppi_create accepts (first 6, last 4, widths 1..256, at most 8
 * entries), theta packed as for mppi_set_nn_params, and the plant's own negate_yaw_der.  n_layers == 0 with theta == NULL clears it:
 * the plant is then the handle's own network with the handle's negate_yaw_der (also the state before the first call).  A
 * basis-function handle: MPPI_ERR_INVALID.  A wrong layer list or n: MPPI_ERR_INVALID, and the plant is what it was.  The model is
 * kept as a host network and as a device image (the image plant_fleet_kernel reads); the call touches no solve state, an armed
 * handle stays armed (the copy uses the device's batch stream: handles armed TOGETHER wait gated on that stream, see
 * mppi_nominal_traj_batch).  A handle's FIRST model allocates the image's device memory, once and for the largest image a layer list
 * can have (1.3 MB, freed with the handle): give a handle its first model before arming it, not beside a gated launch.
 * mppi_debug_plant_model_info: *n_layers = the plant's layer count, 0 without one. */
int mppi_set_plant_model(mppi_handle *h, const int *layers, int n_layers, const float *theta, size_t n, int negate_yaw_der);
int mppi_debug_plant_model_info(const mppi_handle *h, int *n_layers);
/* The drive law.  Inputs per controller: the start state x[7]; a nominal solution state_seq [T][7] and control_seq [T][2] (already
 * clamped: what the nominal calls deliver); optionally the gains feedback [T][2][7] (mppi_get_feedback_gains' layout); periods P
 * with 1 <= P < T; substeps m with 1 <= m <= 16; the plant network and its negate_yaw_der; the handle's float dt and its limits.
 * dt_sub = dt / (float)m, one fp32 division (dt itself at m = 1).  Plant step q = 0 .. P m - 1, lo = q / m, j = q % m, hi = lo + 1,
 * a = (double)j / (double)m:
 *   j == 0: nothing is interpolated -- u_ff, x_des and K are row lo (row hi is not read);
 *   j > 0:  each is (1 - a) v[lo] + a v[hi], evaluated in double as controlAt does; x_des and K are rounded to float, u stays double;
 *   feedback (only when asked for): du[c] = 0, then for i ascending du[c] = fmaf(K[c][i], x[i] - x_des[i], du[c]) in fp32; if
 *           neither du is NaN, u[c] += (double)du[c] (the reference's fallback to feed-forward);
 *   applied control: clamp((float)u[c], u_lo[c], u_hi[c]) with mppi_nominal_traj's clamp and the HANDLE's limits.  The reference
 *           clamps to +-1; the handle's limits are a deliberate deviation: with them the case m = 1 without feedback and without a
 *           plant model IS plant_fleet_kernel's step, i.e. the first P rows of mppi_nominal_traj_batch, bit for bit;
 *   update: one step of mppi_nominal_traj's text on the plant network with dt_sub (the kinematics with fmaf, per neuron the
 *           k-ascending fmaf chain with the bias added afterwards, tanhf, s = fmaf(sd, dt_sub, s)).
 * On the host sin / cos of the heading are sinf / cosf; on the device they are the rounded double results -- the one place the two
 * texts may differ, as in mppi_nominal_traj_batch.
 *
 * mppi_plant_drive_batch: the law for handles[n] from states [n][7], with state_seqs / control_seqs what the nominal calls
 * delivered; states_out [n][7] receives every plant's state after P periods (it may be `states`), applied_log[i] the
 * [periods * substeps][2] applied controls (the array or an entry may be NULL).  With feedback != 0 the gains are each handle's
 * current DDP result; a handle without one: MPPI_ERR_STATE.
 * Order of work and refusals, as in mppi_nominal_traj_batch: every argument is checked first (MPPI_ERR_INVALID: a NULL array other
 * than applied_log, n < 1, a NULL handle or sequence, a handle listed twice, periods outside [1, min T_i), substeps outside
 * [1, 16]), then every handle's readiness (MPPI_ERR_STATE), then pending solves are collected; the outputs are written only after
 * every launch and copy of the call has succeeded.
 * Sharing rule, as mppi_nominal_traj_batch's: n >= 2 handles of the network model with parameters set, all on one device, run in
 * plant_drive_fleet_kernel (one wave per controller; more than 64 handles: launches of up to 64; one input copy, one result copy
 * and one synchronise per call); anything else -- n = 1, a basis-function handle in the set (its plant is its own model), several
 * devices -- runs the host text per handle.  mppi_debug_plant_drive_info tells which it was (*on_device). */
int mppi_plant_drive_batch(mppi_handle *const *handles, const float *states /* n x 7 */, const float *const *state_seqs /* [i]: T_i x 7 */,
                           const float *const *control_seqs /* [i]: T_i x 2 */, int n, int periods, int substeps, int feedback,
                           float *states_out /* n x 7 */, float *const *applied_log /* [i]: periods x substeps x 2, or NULL */);
int mppi_debug_plant_drive_info(const mppi_handle *h, int *on_device);
/* Test hook: the host text of the law for a network given by value -- no handle and no device.  feedback: [T][2][7] or NULL (no
 * feedback; state_seq may then be NULL too); applied: [periods * substeps][2] or NULL.  MPPI_ERR_INVALID for a NULL argument, a
 * layer list mppi_create refuses, n != its parameter count, T < 2, periods outside [1, T), substeps outside [1, 16] or dt <= 0. */
int mppi_debug_plant_drive_host(const int *layers, int n_layers, const float *theta, size_t n, int negate_yaw_der, float dt,
                                const float u_lo[MPPI_CONTROL_DIM], const float u_hi[MPPI_CONTROL_DIM], const float x[MPPI_STATE_DIM],
                                const float *state_seq, const float *control_seq, const float *feedback, int T, int periods, int substeps,
                                float state_out[MPPI_STATE_DIM], float *applied);
/* Closed-loop ticks of a fleet against that plant.  The call is DEFINED as this loop of public calls, which the library also
 * contains (its reference and its fall-back):
 *     for tick in 0 .. n_ticks-1:
 *         mppi_compute_control_batch(handles, s, n)
 *         feedback ? mppi_nominal_and_gains_batch(handles, s, xs, us, n) : mppi_nominal_traj_batch(handles, s, xs, us, n)
 *         mppi_plant_drive_batch(handles, s, xs, us, n, stride, substeps, feedback, s_next, applied)
 *         log s_i, applied_i, the trajectory cost of handle i;  s = s_next;  mppi_slide_control_seq(handle_i, stride)
 * control_log[i] is [n_ticks][stride * substeps][2]; the other logs, the post-conditions on every handle, the order of work and the
 * argument checks are mppi_closed_loop_ticks_batch's, with substeps outside [1, 16] refused as well.
 * Device path (feedback == 0): the sets that take mppi_closed_loop_ticks_batch's device path AND share the launch of
 * mppi_plant_drive_batch.  Every tick is enqueued on the device's batch stream and the host waits for none: behind a tick's tail
 * plant_drive_fleet_kernel reads the device copy of U the tail has just smoothed (it clamps the rows itself: no replay launch is
 * needed), steps the plant from the controller's device state slot and writes the new state into the next tick's rollout argument
 * block, exactly as plant_fleet_kernel does.  Failure: mppi_closed_loop_ticks_batch's check behind the run, and its restore.
 * feedback != 0, and every other set, run the loop above literally, with its bits: a tick whose DDP factorisation fails returns
 * that call's MPPI_ERR_STATE.  mppi_debug_closed_loop_info reports this entry too.  MPPI_CLOSED_LOOP_DEVICE=0 (tools only) applies. */
int mppi_closed_loop_sim_batch(mppi_handle *const *handles, float *states /* n x 7, in: start, out: final */, int n, int n_ticks,
                               int stride, int substeps, int feedback, float *const *state_log /* [i]: (n_ticks+1) x 7, or NULL */,
                               float *const *control_log /* [i]: n_ticks x (stride x substeps) x 2 (applied), or NULL */,
                               float *const *cost_log /* [i]: n_ticks trajectory costs, or NULL */);

/* Host threads the library may use for the host-side work of a tick that comes in pairs (mppi_nominal_traj_pair,
 * mppi_compute_feedback_gains_pair): 1 (default) = the caller's thread only (the reference's optimizer thread does everything,
 * path_integral_main.cu:136-138); 2 = one helper thread, process-wide, which sleeps between ticks and is woken by
 * mppi_compute_control_batch_async.  Results do not depend on the setting. */
int mppi_set_host_threads(int n);

/* MPPICosts::getDebugDisplay without the OpenCV display (costs.cu:272-285 -> debugCostKernel,
 * PI/debug_kernels.cuh:39-88): the costmap around (x, y), width_m x height_m metres at ppm pixels per
 * metre, car marker included; out is [height_m*ppm][width_m*ppm] (n floats), index
 * (H - (yi + 1)) * W + xi as in the reference.  The reference never writes row yi = 0 and flat index
 * 0 (they show whatever the buffer held); here they are 0.  debugDisplayInit's default is 10, 10, 50. */
int mppi_debug_cost_raster(mppi_handle *h, float x, float y, float heading, int width_m, int height_m,
                           int ppm, float *out, size_t n);

/* Measurement hooks.  on = 1: HIP events around every stage of every solve; on = N > 1: only on
 * every Nth solve (event packets between kernels lengthen the launch gaps, so sampling keeps the
 * measured run close to the unmeasured one); on = 0: off. */
int mppi_enable_stage_timing(mppi_handle *h, int on);
int mppi_reset_stage_times(mppi_handle *h);
int mppi_get_stage_times(mppi_handle *h, mppi_stage_times *out);
/* Name of the rollout kernel form in use, and mppi_set_rollout_variant's names for forcing one.  What is LOAD-BEARING:
 *
 *   automatic choice (csrc/abi_forms.hip: kFormRules, by model shape and 16-rollout groups per CU)
 *     "row_tree"         valu_row8w_tree_h32_l2             6-32-32-4, K <= 8192: the headline form (vector ALU; output layer a butterfly)
 *     "m44"              mfma4x4x1_h64_l<N>_m44_split_tree  64-wide nets, K <= 8192 (hidden layers as two chains, output a butterfly)
 *     "quad"             mfma16x16x4_h<H>_l<N>_quad4w       other shapes up to one group per CU (e.g. 6-32x4-4), and under "mfma"
 *     "multi2"           ..._multi2                         up to two groups per CU
 *     "multi4_tree_gen"  ..._multi4_tree_gen                beyond (BASELINE config 4; eps from the stand-alone generator kernel)
 *     "fused"            ..._fused_b256                     shapes without a multi form beyond two groups per CU (6-64x4-4, K > 8192)
 *     (generic)          valu_lds                           any other layer list: the only form for non-uniform nets
 *     basis functions    basis_funcs25_valu[_2w|_3w]        "fused" | "quad" | "bf3"
 *   the basis-function model by name only (the bits of the three forms above)
 *     "bf_row"           basis_funcs25_row8w                a rollout's 16 (output, y-thread) cells on one DPP row, four dynamics
 *     wavefronts + pose, cost, control and noise wavefront per 16 rollouts (the row form's group); K a multiple of 16; the model's
 *     only form with a gated kernel (mppi_arm, mppi_arm_batch for a pair, chained mppi_control_ticks); MPPI_ERR_UNSUPPORTED on a
 *     network handle
 *   the reference's summation order in EVERY layer (bit-identical to one another; "mfma" = the table restricted to them)
 *     "row_exact" (= "row") valu_row8w_h32_l2, "m44_chain" mfma4x4x1_*_m44_tree (hidden layers one chain; output a butterfly),
 *     "oct[_gen]" ..._oct8w, "quad", "multi2[_gen]", "multi4[_gen]", "fused" = "block256" | "block64" ..._fused_b256 / _b64,
 *     "lds44" mfma4x4x1_lds_l<hidden layers>_w<widest hidden layer>: ANY layer list 6 -> hidden widths 1..64 -> 4 (the standard
 *     shapes included) in the latency regime -- the m44 group with the weights of every layer read from LDS and the output layer
 *     as one more chain; by name only (never chosen automatically); has a gated form (mppi_arm, chained mppi_control_ticks);
 *     MPPI_ERR_UNSUPPORTED for the basis-function model, a hidden width above 64, or a list without a hidden layer
 *     "lds128" mfma4x4x1_lds2h_l<hidden layers>_w<widest hidden layer>: the same for hidden widths 1..128 -- a layer is one or
 *     two halves of 64 neurons with an accumulator each, its inputs walked k ascending over one or two activation sets; the
 *     weight image must fit a workgroup's 160 KB of LDS beside 34 KB of rings (6-128-128-4: 141 KB; 6-128-128-128-4 does not);
 *     by name only; gated form as "lds44"; lists up to 64 wide are accepted and give "lds44"'s bits, but belong to "lds44";
 *     MPPI_ERR_UNSUPPORTED for the basis-function model, a hidden width above 128, a list without a hidden layer, or an
 *     image that does not fit (the message states needed and available bytes)
 *     "lds16" mfma16x16x4_lds_l<hidden layers>_w<widest hidden layer>: the THROUGHPUT form of the same lists (hidden widths 1..128) --
 *     "fused"'s wavefront (16 rollouts, the whole step, v_mfma_f32_16x16x4, eps from the stand-alone generator kernel) with the
 *     layer list a kernel argument and the weights read from an LDS image per workgroup (6-128-128-128-4: 144 KB, fits; a fourth
 *     128-wide layer does not); workgroups of 256 / 512 / 1024 threads, the smallest with every workgroup resident at once; by
 *     name only; NO gated form (mppi_arm answers MPPI_ERR_UNSUPPORTED) and no batched launch (a batch solves handle by handle);
 *     MPPI_ERR_UNSUPPORTED as "lds128"
 *     "fleet16" mfma16x16x4_fleet_l<hidden layers>_w<widest hidden layer>: "lds16"'s wavefront, image and lists (hidden widths 1..128,
 *     the image fits 160 KB of LDS; the same refusals) with the argument block read from device memory, so that up to 64 handles of
 *     one layer list share ONE rollout launch (mppi_compute_control_batch: the sharing rule is stated there); the bits of "lds16"
 *     and "valu_lds"; NO gated form; a handle solved alone runs the same kernel with one instance; by name only.
 *     "fleet_multi4" mfma16x16x4_h<H>_l<N>_fleet_multi4_tree_gen: "multi4_tree_gen"'s workgroup (four dynamics waves with every
 *     weight in registers, riders on the side, the output layer as a butterfly, eps from the stand-alone generator kernel) with the
 *     argument block read from device memory, so that up to 64 handles of one shape share ONE rollout launch
 *     (mppi_compute_control_batch: the sharing rule is stated there); the bits of "multi4_tree_gen"; the fleet form to ask for on
 *     these shapes (ahead of "fleet16" at every fleet size, ahead of "auto" from 16 handles on); NO gated form; a
 *     handle solved alone runs the same kernel with one instance; by name only; MPPI_ERR_UNSUPPORTED for the basis-function model
 *     and for any list but 6-32x2-4, 6-32x4-4, 6-64x2-4 (K is a multiple of 64 on every handle: mppi_create).
 *     "fleet_bf" basis_funcs25_fleet (the basis-function model only): the model's own workgroups -- one, two or three waves per
 *     64 rollouts, the bodies of basis_funcs25_valu / _2w / _3w -- with the argument block read from device memory and eps from
 *     the stand-alone generator kernel, so that up to 64 handles share ONE rollout launch (mppi_compute_control_batch: the
 *     sharing rule is stated there); the bits of "bf3".  One wave count per launch, chosen by the rule of a single handle with the
 *     64-rollout groups counted over the fleet (three waves while 3 x groups <= SIMDs, two while groups <= SIMDs, else one);
 *     "fleet_bf_w1" / "fleet_bf_w2" / "fleet_bf_w3" (basis_funcs25_fleet_w<N>) force the count.  NO gated form; a handle solved
 *     alone runs the same kernel with one instance; by name only; MPPI_ERR_UNSUPPORTED for the network model.
 *     "glb16" mfma16x16x4_glb_l<hidden layers>_w<widest hidden layer>: "lds16"'s wavefront for EVERY layer list of the network model
 *     (3 <= n_layers <= 8, hidden widths 1..256): the same image with up to 16 tiles per layer; its head (biases, layer 0) and the
 *     first R of its 1 KB blocks are copied into LDS, the other blocks are read from the image in global memory (it stays in L2),
 *     R = what fits 160 KB; "glb16_r<N>" (N decimal, >= 0) caps R at N ("glb16_r0": every block from global memory; a test and
 *     measurement knob, same bits for every N); by name only; the device image is built at this call and held only by handles
 *     that asked for the form; NO gated form and no batched launch, as "lds16"; MPPI_ERR_UNSUPPORTED for the basis-function
 *     model and a list without a hidden layer, MPPI_ERR_INVALID ("unknown variant") for a malformed suffix
 *     "fleet_glb16" mfma16x16x4_fleet_glb_l<hidden layers>_w<widest hidden layer> (of the handle's OWN list): "glb16"'s wavefront, image,
 *     residency rule and lists with the argument block and the layer list read from device memory, so that up to 64 handles of
 *     ANY layer lists share ONE rollout launch (mppi_compute_control_batch: the sharing rule is stated there); the bits of
 *     "valu_lds", "glb16" and, where it takes the list, "lds16".  One kernel instance per launch: 16 tiles per layer if any handle of
 *     the launch has a hidden layer wider than 128, else 8 (a narrower list skips the upper tiles: same bits); every handle keeps
 *     the R of a launch of its own, the launch's dynamic LDS is the largest of the handles'.  "fleet_glb16_r<N>" caps the handle's
 *     R at N as "glb16_r<N>" does (same bits for every N; the caps of a launch need not agree).  NO gated form; a handle solved
 *     alone runs the same kernel with one instance; by name only; the refusals of "glb16"
 *     "glb44" mfma4x4x1_glb_l<hidden layers>_w<widest hidden layer>: "lds128"'s group (512 threads per 16 rollouts, four dynamics
 *     waves on v_mfma_f32_4x4x1 + the riders) for EVERY layer list of the network model (3 <= n_layers <= 8, hidden widths 1..256): a
 *     layer is one to four halves of 64 neurons with an accumulator each, the reference's order (the bits of "valu_lds", "lds128" and
 *     "glb16"); the head of the image (biases, layer 0) and the first R of its 1 KB quads are copied into LDS behind the group's
 *     shared state, the other quads are read from the image in global memory, R = what fits 160 KB; "glb44_r<N>" caps R at N (a
 *     test and measurement knob, same bits for every N); by name only; the device image is built at this call and held only by
 *     handles that asked for the form; it HAS a gated form (mppi_arm, chained mppi_control_ticks) and two handles forced to it
 *     with the same whole layer list and the same cap share one launch (mppi_compute_control_batch, mppi_arm_batch);
 *     MPPI_ERR_UNSUPPORTED for the basis-function model and a list without a hidden layer, MPPI_ERR_INVALID ("unknown variant")
 *     for a malformed suffix
 *     "row32" valu_row8w_l<hidden layers>_w<widest hidden layer>: the ROW form ("row_exact"'s group: the network on the vector ALU, a
 *     rollout on a 16-lane DPP row, every weight in registers) for ANY layer list 6 -> ONE TO THREE hidden widths 1..32 -> 4; a
 *     hidden layer narrower than 32 runs as a 32-wide one whose missing neurons have weight 0 and bias 0 (the padded inputs come
 *     last in every chain: the reference's order and the bits of "valu_lds" / "lds44"; only the sign of a pre-activation that is
 *     exactly zero can differ); on 6-32-32-4 the bits and the kernels of "row_exact".  The latency form to ask for on these lists:
 *     K = 1920, T = 100 (us) 6-32-4 32, 6-16-24-4 41, 6-32-32-32-4 55 beside "lds44" 65 / 88 / 156.  By name only;
 *     the device image is built at this call and held only by handles that asked for the form; it HAS a gated form (mppi_arm,
 *     chained mppi_control_ticks) and two handles forced to it with the same whole layer list share one launch
 *     (mppi_compute_control_batch, mppi_arm_batch; three or four solve one by one).  From three hidden layers on a group's
 *     registers leave room for ONE group per CU: K above 16 x CUs runs in rounds -- correct, and not what the form is for.
 *     MPPI_ERR_UNSUPPORTED for the basis-function model, a hidden width above 32, no or more than four hidden layers, and for FOUR
 *     hidden layers (the fourth layer's weights do not fit the registers in this order: "row32_tree" serves such a list)
 *   re-associated, by name only
 *     "row32_tree" valu_row8w_tree_l<hidden layers>_w<widest hidden layer>: "row32" with the output layer as "row_tree"'s butterfly,
 *     for ONE TO FOUR hidden widths 1..32: the reference's order in the hidden layers, inside the 1e-4 tolerance on the controls as
 *     "row_tree" is; on 6-32-32-4 the bits and the kernels of "row_tree".  K = 1920, T = 100 (us): 6-32-4 26, 6-16-24-4 33,
 *     6-32-32-32-4 47, 6-32x4-4 61 -- 6-32x4-4 runs "quad" automatically at 118, and has no gated form there.  Image, gated form,
 *     pair launch, residency and refusals as "row32", four hidden layers accepted
 *   A/B arms and cross-checks (never chosen automatically)
 *     "valu" valu_reg_lds (lane = rollout, the independent implementation every parity test also runs; config 4's untuned
 *     vector-ALU reference), "valu_lds" (the generic kernel on a standard shape), "row64" = "row64_r16"
 *     valu_row64_r16_tree_h64_l<N> (config 4's hand-scheduled vector-ALU arm), "multi4_tree" (in-kernel generator)
 *   "auto" restores the table.  "mfma", "valu", "valu_lds" also drop a form forced by name earlier.
 * The re-associated forms ("_tree", "_split") do NOT compute the reference's summation order: inside the 1e-4 tolerance on
 * the controls (profiles/r05_b_nominal_margin_*.txt), not bit-identical to the exact ones.  Removed in ABI 5 (no table row chose
 * them, no A/B needed them): "multi1", "multi4u[_gen]", "row64_r8".  MPPI_ERR_UNSUPPORTED if the handle's model has no such
 * form; a form name given to a handle whose model runs on the generic vector kernel is accepted and ignored. */
const char *mppi_rollout_variant(const mppi_handle *h);
int mppi_set_rollout_variant(mppi_handle *h, const char *name);

/* Test hook (not part of the drop-in surface): d/dt of n independent (state[7], control[2])
 * pairs through the SAME device functions the rollout kernel uses (computeKinematics +
 * computeDynamics, neural_net_model.cu:346-410); ders is [n][7]. */
int mppi_debug_dynamics(mppi_handle *h, int n, const float *states, const float *controls, float *ders);

/* Test hook (not part of the drop-in surface): from the next solve on, wavefront role `wave` of the
 * multi-wavefront rollout kernels starts with an exhausted poll budget, i.e. it never waits for its
 * partners -- the state of a wave that gave up on a hand-over -- and every other wave may spend
 * spin_budget + 64 T polls in total (0: the default).  Roles of the four-wavefront network kernel: 1, 2 =
 * dynamics waves, 3 = cost wave, 4 = control wave; of the two-wavefront basis-function kernel: 1 = dynamics,
 * 2 = cost.  The solve must then end in MPPI_ERR_HIP ("hand-over failed"), never in finite costs.
 * wave = 0 and spin_budget = 0 restore normal operation.
 * Roles of the row form, of "bf_row" and of the oct form: 1 .. 4 = dynamics waves, 5 = pose, 6 = cost, 7 = control, 8 = noise wave.
 * Roles of the multi form: 1 .. ND = dynamics waves, then the cost wave and the control wave (ND = 4: the pose
 * wave, the cost wave, the control wave).
 * Roles 32 .. 34: waits of the one-launch tail kernel of solves with more than 4096 rollouts -- the weights workgroup of
 * chunk 0 never publishes its chunk sum of weights (32), chunk 0 of every row never publishes its chain results (33), no
 * weights workgroup publishes its chunk sum, nor beta where the tail kernel takes the minimum itself (34) -- with a deadline of spin_budget microseconds for every wait (0: the default, 20 ms). */
int mppi_debug_inject_handover_fault(mppi_handle *h, int wave, int spin_budget);

/* Test hooks (not part of the drop-in surface): what EVERY iteration of a solve with num_iters > 1 left behind.  The
 * reference's iteration loop (PI/mppi_controller.cu:609-667) re-uses U_ -- the raw weighted mean, unsmoothed -- as the
 * nominal sequence of the next iteration, so from iteration 2 on a comparison with another implementation is a
 * comparison on identical inputs only if that implementation is started from THIS one's U of the iteration before.
 * mppi_debug_capture_iterations(h, 1): from the next solve on, keep them (two small device copies per iteration; such a
 * handle is solved on its own, never inside a batched launch); 0: off.
 * mppi_debug_get_iterations: U_raw [num_iters][T][2] = the weighted mean after iteration i before any smoothing
 * (weightedReductionKernel's output, :219-267), costs [num_iters][K], V [num_iters][K][T][2] = the applied controls
 * (explicit-noise solves only: MPPI_ERR_STATE otherwise); each may be NULL. */
int mppi_debug_capture_iterations(mppi_handle *h, int on);
int mppi_debug_get_iterations(mppi_handle *h, float *U_raw, float *costs, float *V);

/* Test / tooling hook (not part of the drop-in surface): the kernel forms the library's selection table knows for this
 * handle's model, as names for mppi_set_rollout_variant, the table's order; returns how many were written (<= max_n).
 * tests/test_form_selection_gpu.py times them against the automatic choice. */
int mppi_debug_form_candidates(const mppi_handle *h, const char **names, int max_n);

/* Test / tooling hook (not part of the drop-in surface): mppi_control_ticks on one handle in the row form enqueues every
 * solve but the first one tick AHEAD, gated on a word the host writes once it holds the previous result (csrc/abi_solve.hip:
 * chained control ticks; the launch call and the dispatch leave the step's critical path); on = 0 launches every solve when
 * its turn comes.  The results are bit for bit the same. */
int mppi_debug_set_chained_ticks(mppi_handle *h, int on);

/* Test / tooling hook.  In solves of more than 8192 rollouts (the rollout forms of csrc/rollout_multi.hip with the one-launch
 * tail kernel of K > 4096) the rollout kernel leaves beta = min_k costs[k]
 * (mppi_controller.cu:630-634, computeNormalizer's baseline: exact, order-free) behind as a tagged atomic minimum and the tail
 * kernel reads it instead of reducing the costs and handing the result round (csrc/mppi_device.hpp: publish_min_cost); a rollout
 * form that does not publish, or costs without one finite value, make the tail kernel reduce them itself.  Same bits either way.
 * on = 0 / 1 switches the publication off / on (default on; on < 0 leaves it); *from_rollout (may be NULL) receives whether the
 * LAST solve's tail kernel took beta from the rollout kernel (0 where the rollout form does not publish: by default every solve
 * of <= 8192 rollouts). */
int mppi_debug_min_cost(mppi_handle *h, int on, int *from_rollout);

/* Test / tooling hook: *instances = how many instances the rollout launch of this handle's most recently ENQUEUED solve served
 * (an armed solve that is not yet opened counts; 1: a launch of its own; 2..64: shared with the other handles of a
 * mppi_compute_control_batch / mppi_arm_batch call; 0: no solve yet), *gated = 1 if that launch was a gated one (mppi_arm,
 * mppi_arm_batch, the chained mppi_control_ticks).  Recorded where the launch is made.  MPPI_ERR_INVALID for a NULL argument. */
int mppi_debug_launch_info(mppi_handle *h, int *instances, int *gated);

/* How long a blocking call (mppi_compute_control, mppi_synchronize, mppi_get_results ...) polls for a solve's result block
 * before it gives up with MPPI_ERR_HIP; default 30 s.  (The reference blocks in cudaStreamSynchronize without a limit,
 * PI/mppi_controller.cu:667; at 50 Hz a controller may want a limit of a few periods.)  The clock is read every 256 polls,
 * so the limit holds to microseconds.  After a timeout the lost solve is never waited for again: the control sequence and
 * history the host holds (what mppi_get_control_seq returns: the state before the lost solve) are what the next solve
 * starts from; while the lost solve's device work is still running every solve entry and result getter returns
 * MPPI_ERR_HIP at once (one hipStreamQuery, no blocking), and the handle works again once that work has drained.
 * mppi_destroy synchronises the handle's streams: it may block for as long as that work runs. */
int mppi_set_wait_timeout(mppi_handle *h, double seconds);

#ifdef __cplusplus
}
#endif
#endif /* MPPI_HIP_H_ */
