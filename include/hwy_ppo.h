/*
 * hwy_ppo.h -- C ABI of the fused PPO minibatch step (libhwy.so).
 *
 * Replaces, for the batched path, the per-minibatch body of PPOAgent.update
 * (reference ppo/agent.py:216-252): ActorCritic.evaluate (:76-84) on the minibatch, the
 * ratio / KL / clipped surrogate / MSE / entropy loss (:226-245), loss.backward(),
 * clip_grad_norm_(0.5) (:249-251) and Adam.step() (:252, torch.optim.Adam defaults).
 * hwy_ppo_act replaces the acting forward and sampling on the batched rollout path (below);
 * hwy_ppo_value_masked replaces nothing there: it is ActorCritic.forward's value (:46-54) on the final
 * observations of the truncated rows only, for the opt-in bootstrap at a time limit that the
 * reference, which books truncation as terminal (training/routine.py:135), does not have.
 *
 * Network (ppo/agent.py:23-42): shared = Lin(S,H)-ReLU-Lin(H,H)-ReLU; actor_mean =
 * Lin(H,H)-ReLU-Lin(H,A); log_std[A]; critic = Lin(H,H)-ReLU-Lin(H,1).  Parameters live in
 * one flat fp32 buffer in nn.Module.parameters() order:
 *   shared.0.{weight,bias} shared.2.{weight,bias} actor_mean.0.{weight,bias}
 *   actor_mean.2.{weight,bias} log_std critic.0.{weight,bias} critic.2.{weight,bias}
 * (weights [out, in] row-major, as nn.Linear stores them).
 *
 * All math is fp32; GEMMs use v_mfma_f32_16x16x4_f32 / v_mfma_f32_32x32x2_f32 (exact fp32
 * products, fp32 accumulate).
 * Calls are asynchronous, allocate nothing and are hipGraph-capturable.
 *
 * Weight tile image: on the fused path (S % 4 == 0, S <= 1024, H <= 512) the row kernel streams
 * the weights from a tiled copy kept in the workspace.  (Past S = 256 the row and act kernels run
 * their first layer over chunks of 256 state columns, always at 16-row tiles; every other shape
 * outside the fused range takes the general path.)  hwy_ppo_optimizer rewrites it with every
 * Adam step; call hwy_ppo_sync_params once before the first hwy_ppo_forward_backward on a
 * workspace, and again whenever params were written by anything other than hwy_ppo_optimizer
 * (a checkpoint load, a torch optimizer step, a broadcast).
 *
 * Memory contract.  The workspace is hwy_ppo_workspace_bytes(dims) bytes of device memory
 * and may contain ARBITRARY bytes before the first hwy_ppo_sync_params: no call
 * needs it zeroed, and none reads a word of it that the same call sequence has not written.  The
 * only state it carries from one call to the next is the weight tile image (the last
 * workspace bytes from hwy_ppo_tile_image_offset on; none on the general path) and, from a
 * hwy_ppo_forward_backward to the hwy_ppo_optimizer of the same step with grads_modified == 0, the
 * gradient-norm partials: every other byte may be overwritten between steps, and with
 * grads_modified == 1 between the two calls of a step as well.  hwy_ppo_forward_backward writes
 * the whole flat gradient (what grads held before does not matter) and one metrics row.  No call
 * writes outside the buffers it is given, each taken at exactly the size this header states
 * (states [n, S] with n > B rows, idx [B], the outputs of hwy_ppo_act [B] rows, the device tables
 * and the control block exactly their *_bytes), and none writes a buffer declared const here or
 * an output it was not asked for.  tests/test_ppo_memory_gpu.py runs the step, acting, grouped,
 * mixed, scheduled and control calls under these conditions: between guard words, on a workspace
 * poisoned with NaNs and with FLT_MAX, bit for bit against a zeroed one
 * (tests/test_input_grad_gpu.py guards hwy_ppo_input_grad).
 */
#ifndef HWY_PPO_H_
#define HWY_PPO_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hwy_ppo_dims {
  int32_t B; /* minibatch rows */
  int32_t S; /* state_dim */
  int32_t H; /* hidden_dim (multiple of 64) */
  int32_t A; /* action_dim (2) */
} hwy_ppo_dims;

/* Flat-parameter offsets (floats) for dims; numel returned. */
int hwy_ppo_param_layout(const hwy_ppo_dims* d, int64_t* offsets /*[13]*/, int64_t* numel);
/* Workspace bytes needed by hwy_ppo_forward_backward / hwy_ppo_optimizer for dims. */
int64_t hwy_ppo_workspace_bytes(const hwy_ppo_dims* d);

typedef struct hwy_ppo_args {
  hwy_ppo_dims dims;
  /* rollout sources (flattened [n, ...]) and this minibatch's row indices [B] (int64) */
  const float* states;    /* [n, S] */
  const float* pre_tanh;  /* [n, A] */
  const float* old_logp;  /* [n] */
  const float* adv;       /* [n] normalised advantages */
  const float* ret;       /* [n] returns */
  const int64_t* idx;     /* [B] */
  /* model / optimizer state (flat, hwy_ppo_param_layout order) */
  float* params;
  float* grads;
  float* adam_m;
  float* adam_v;
  int32_t* counters;      /* [0] Adam step t, [1] metrics row */
  float* metrics;         /* [rows, 6]: policy, value, entropy, loss, clip count, kl */
  void* workspace;        /* hwy_ppo_workspace_bytes(dims) bytes, owned by these calls; arbitrary
                             contents before hwy_ppo_sync_params (memory contract, above) */
  /* hyper-parameters (PPOAgent defaults: eps_clip .2, value_coef .5, entropy_coef .005) */
  float eps_clip, value_coef, entropy_coef, max_grad_norm;
  float lr, beta1, beta2, adam_eps;
  int32_t grads_modified; /* grads changed after forward_backward (e.g. all-reduced): the
                             optimizer recomputes the gradient norm from them */
} hwy_ppo_args;

/* Forward, loss, backward: writes grads (flat) and the metrics row. */
int hwy_ppo_forward_backward(const hwy_ppo_args* a, void* stream);
/* clip_grad_norm_(max_grad_norm) + Adam step on params (call after any gradient all-reduce). */
int hwy_ppo_optimizer(const hwy_ppo_args* a, void* stream);
/* Measurement aid (bench.py's per-kernel roofline): each kernel of the minibatch step
 * (ppo_rows, ppo_wgrad, ppo_wsum, ppo_adam) captured as a HIP graph of `reps` back-to-back
 * launches on a private stream and replayed between two events; writes the average microseconds
 * per launch to us[0..3], and to us[4] the same for an empty one-workgroup kernel (the launch
 * floor a kernel-trace duration leaves out).  The Adam launches update params / moments / the tile image as training
 * steps do; the Adam step count is restored and the metrics row index left at 0.  Waits for
 * `stream` first; synchronous, not graph-capturable; fused path, grads_modified == 0.
 * -1 bad args, -2 HIP error. */
int hwy_ppo_time_kernels(const hwy_ppo_args* a, void* stream, int reps, float* us);
/* Rebuild the workspace's weight tile image from params (uses dims, params, workspace). */
int hwy_ppo_sync_params(const hwy_ppo_args* a, void* stream);

/* Byte offset of the weight tile image inside a workspace for dims (-1 when the dims take
 * the general path, which keeps none).  The image depends on S and H only. */
int64_t hwy_ppo_tile_image_offset(const hwy_ppo_dims* d);

/* ActorCritic.act on a batch (replaces ppo/agent.py:86-95's forward + Normal sample + tanh +
 * squashed log-prob on the batched rollout path): dims.B rows of states [B][S] (contiguous);
 * noise [B][2] standard-normal draws (the caller's generator, as act() draws them) or NULL for
 * act(deterministic=True) (z = mean, log_prob = 0).  Needs S % 4 == 0, S <= 1024,
 * H in {64, 128, ..., 512}.  tiles: NULL, or the tile image of a hwy_ppo workspace with the same
 * S and H that is in step with params (workspace + hwy_ppo_tile_image_offset; current after
 * hwy_ppo_optimizer / hwy_ppo_sync_params until params are written by anything else): the
 * forward then streams whole 1-KB operand tiles instead of 64-B pieces of params rows. */
typedef struct hwy_ppo_act_args {
  hwy_ppo_dims dims;
  const float* states;
  const float* params; /* flat, hwy_ppo_param_layout order */
  const float* noise;
  float* action;   /* [B][2] tanh(z) */
  float* pre_tanh; /* [B][2] z */
  float* logp;     /* [B] */
  float* value;    /* [B] */
  const float* tiles; /* optional weight tile image (see above), or NULL */
} hwy_ppo_act_args;
int hwy_ppo_act(const hwy_ppo_act_args* a, void* stream);

/* The critic's value of the truncated rows only (replaces nothing in the reference, which books a
 * time limit as terminal, training/routine.py:135; it is the V(final observation) that the
 * bootstrap at truncation, hwy_gae_boot, needs).  Row b is marked iff truncated[b] &&
 * !(terminated && terminated[b]) (both [B] u8, terminated nullable).  value[b] = the value
 * hwy_ppo_act computes for states row b (the same kernel body for the same dims and tiles, so the
 * same bits) for a marked row and exactly 0.0f for any other; a 16- or 32-row tile without a
 * marked row stores its zeros and returns before it reads a weight.  Nothing else is written:
 * a->action / pre_tanh / logp may be NULL, a->noise must be NULL.  -1 for bad arguments or dims
 * hwy_ppo_act refuses, before any device call. */
int hwy_ppo_value_masked(const hwy_ppo_act_args* a, const uint8_t* truncated,
                         const uint8_t* terminated /*nullable*/, void* stream);

/* ---- Grouped learners: G independent learners (a sweep cell's seeds, or the cells of one
 * hidden width; ppo/group.py, ExperimentRunner.launch_group; the reference runs them as separate processes,
 * experiments/runner.py:46-155 under main.py:188-242's joblib / SLURM fan-out) stepped in ONE
 * launch per kernel.  Workgroup (x, y) runs the solo launch's workgroup x for learner y, whose
 * kernel arguments the kernels read from a device table; the kernel bodies and tile shapes are
 * the solo calls', so each learner's results are bit for bit its solo run's.  The *_prepare
 * calls build a table from G argument structs (synchronous: they wait for `stream`; not
 * capturable); the launch calls are asynchronous and hipGraph-capturable.
 *
 * hwy_ppo_group_step = hwy_ppo_forward_backward + hwy_ppo_optimizer for every learner (fused
 * path with 16-row tiles, i.e. minibatches below 64 x CUs rows; grads_modified == 0; 16-byte
 * aligned flat buffers).  The learners share B and H; their state dims S may differ (e.g. the
 * h256 cells of a sweep: no PE S = N*F, RankPE / DistPE S = N*(F+d)): each launch covers the
 * largest learner's grid (the plan prepare writes) and a learner's surplus workgroups exit.
 * hwy_ppo_group_table_bytes depends on B, H and G only.  -1 bad arguments / unsupported dims,
 * -2 HIP error.
 *
 * Wide states: when a learner of the table has S > 256, the row (or act) launch runs the chunked
 * kernels for every learner it covers -- at S <= 256 they run one chunk and produce the narrow
 * kernels' bits -- and prepare marks that in the plan by setting HWY_PPO_PLAN_WIDE in grid_rows
 * (hwy_ppo_mixed_plan / hwy_ppo_sched_plan: in grid_rows[c] of the class; hwy_ppo_mixed_act_plan:
 * in lds_bytes[c]); the value itself is the field without that bit. */
#define HWY_PPO_PLAN_WIDE (1 << 30)
typedef struct hwy_ppo_group_plan {
  int32_t G, B, H;                                    /* learners; shared minibatch rows, hidden */
  int32_t grid_rows, grid_wgrad, grid_wsum, grid_adam; /* each launch's grid: the largest learner's */
} hwy_ppo_group_plan;
int64_t hwy_ppo_group_table_bytes(const hwy_ppo_dims* d, int G);
int hwy_ppo_group_prepare(const hwy_ppo_args* a /*[G]*/, int G, void* table,
                          hwy_ppo_group_plan* plan, void* stream);
int hwy_ppo_group_step(const hwy_ppo_group_plan* plan, const void* table, void* stream);
/* hwy_ppo_act for G learners (same B and H; S may differ); `tiles` = whether the learners' args
 * carry tile images (all or none), which picks the solo call's kernel.  hwy_ppo_group_act's d
 * carries the shared B and H and the LARGEST S of the learners (S > 256: the chunked kernels). */
int64_t hwy_ppo_group_act_table_bytes(int G);
int hwy_ppo_group_act_prepare(const hwy_ppo_act_args* a /*[G]*/, int G, void* table, void* stream);
int hwy_ppo_group_act(const hwy_ppo_dims* d, int G, int tiles, const void* table, void* stream);

/* ---- Grouped learners of different hidden widths: the grouped calls above for learners that
 * share B and A while H and S vary per learner (a sweep across hidden_dim in one set of
 * launches).  The weight-gradient, slice-sum and Adam launches read each learner's H from the
 * table; the row and act kernels read learner y's width class and run the solo kernel's body for
 * it, so each learner stays bit for bit its solo run.  The solo kernels run 8 waves for
 * H = 128, 256, 384, 512 (class 0) and 4 waves for H = 64, 192, 320, 448 (class 1); a launch covers
 * one class, so a table holding both issues two row (or act) launches, each skipping the other
 * class's learners.  The kernels take their LDS as dynamic LDS sized to the widest learner of the
 * class (lds_bytes; prepare raises the kernels' dynamic-LDS limit, never a launch).
 *
 * Every learner must satisfy what hwy_ppo_group_prepare asks of one (fused path, 16-row tiles,
 * grads_modified == 0, 16-byte aligned flat buffers).  Prepare is synchronous (it waits for
 * `stream`) and not capturable; hwy_ppo_mixed_step / hwy_ppo_mixed_act are asynchronous, allocate
 * nothing and are hipGraph-capturable.  -1 bad arguments / unsupported dims, -2 HIP error. */
typedef struct hwy_ppo_mixed_plan {
  int32_t G, B;              /* learners; shared minibatch rows */
  int32_t present[2];        /* learners of wave-count class 0 (8 waves) / 1 (4 waves): 0 = none */
  int32_t grid_rows[2];      /* each class's row grid */
  int32_t lds_bytes[2];      /* each class's dynamic LDS: its widest learner's images */
  int32_t grid_wgrad, grid_wsum, grid_adam; /* the largest learner's */
} hwy_ppo_mixed_plan;
int64_t hwy_ppo_mixed_table_bytes(const hwy_ppo_dims* d /*[G]*/, int G);
int hwy_ppo_mixed_prepare(const hwy_ppo_args* a /*[G]*/, int G, void* table,
                          hwy_ppo_mixed_plan* plan, void* stream);
/* hwy_ppo_forward_backward + hwy_ppo_optimizer for every learner: one row launch per class
 * present, then one launch each of the weight-gradient, slice-sum and Adam kernels. */
int hwy_ppo_mixed_step(const hwy_ppo_mixed_plan* plan, const void* table, void* stream);
/* hwy_ppo_act for G learners of different H (and S); all carry tile images or none do, all carry
 * noise or none do; B below the 32-row-tile threshold (64 x CUs).  Each learner runs the kernel
 * body its solo hwy_ppo_act call runs (with tile images H = 256 takes the compact one). */
typedef struct hwy_ppo_mixed_act_plan {
  int32_t G, B, tiles;       /* learners; rows per learner; tile images carried */
  int32_t present[2];        /* as hwy_ppo_mixed_plan */
  int32_t lds_bytes[2];
} hwy_ppo_mixed_act_plan;
int64_t hwy_ppo_mixed_act_table_bytes(int G);
int hwy_ppo_mixed_act_prepare(const hwy_ppo_act_args* a /*[G]*/, int G, void* table,
                              hwy_ppo_mixed_act_plan* plan, void* stream);
int hwy_ppo_mixed_act(const hwy_ppo_mixed_act_plan* plan, const void* table, void* stream);

/* ---- Grouped learners with schedules of their own: G learners stepped through one WHOLE update
 * when, besides H and S, their minibatch rows B, minibatches per epoch nmb and epochs differ (a
 * sweep across batch_size and epochs in one set of launches).  Slot s of an update is its s-th
 * grouped step.  Learner y is active in slot s iff s < steps[y] = epochs[y] * nmb[y], and then
 * runs its solo step (hwy_ppo_forward_backward + hwy_ppo_optimizer) for minibatch s % nmb[y]:
 * epoch-major, minibatch-minor, the order of a solo update.  A learner that sits a slot out is not
 * touched at all (parameters, gradients, moments, tile image, counters, metrics rows), so its
 * counters[1] ends the update at steps[y]; each active learner is bit for bit its solo run.
 *
 * a[g].idx points at learner g's WHOLE permutation, nmb[g] * B_g indices; minibatch i reads
 * idx + i * B_g.  Every learner must satisfy what hwy_ppo_mixed_prepare asks of one (fused path,
 * 16-row tiles, grads_modified == 0, 16-byte aligned flat buffers, the same A); B may differ.
 *
 * The schedule lives in the device table: the step kernels take the slot as slot base + `slot`,
 * the slot base a word of the table that hwy_ppo_sched_begin zeroes and hwy_ppo_sched_advance
 * adds to, `slot` a launch argument.  One captured graph of P slots -- hwy_ppo_sched_step(slot =
 * 0..P-1), then hwy_ppo_sched_advance(P) -- replayed ceil(max_steps / P) times after one
 * hwy_ppo_sched_begin therefore runs the update for any P; with P = plan.period (or a divisor)
 * no learner ends inside a replay, and slots past max_steps do nothing.  The step kernels only
 * read the slot base; begin (a memset) and advance (one thread's ordinary store) write it,
 * stream-ordered between whole slots.
 *
 * hwy_ppo_sched_prepare is synchronous (it waits for `stream`), leaves the slot base at 0 and is
 * not capturable; begin, step (slot >= 0) and advance (slots >= 0) are asynchronous, allocate
 * nothing and are hipGraph-capturable.  A step issues a row launch per wave-count class present,
 * then the weight-gradient, slice-sum and Adam launches.  -1 bad arguments / unsupported dims,
 * -2 HIP error. */
typedef struct hwy_ppo_sched_plan {
  int32_t G;
  int32_t present[2], grid_rows[2], lds_bytes[2]; /* as hwy_ppo_mixed_plan */
  int32_t grid_wgrad, grid_wsum, grid_adam;
  int32_t max_steps; /* max over learners of epochs * nmb */
  int32_t period;    /* gcd of the learners' steps: every learner ends on a multiple of it */
} hwy_ppo_sched_plan;
int64_t hwy_ppo_sched_table_bytes(const hwy_ppo_dims* d /*[G]*/, const int32_t* nmb /*[G]*/, int G);
int hwy_ppo_sched_prepare(const hwy_ppo_args* a /*[G]*/, const int32_t* nmb /*[G]*/,
                          const int32_t* epochs /*[G]*/, int G, void* table,
                          hwy_ppo_sched_plan* plan, void* stream);
int hwy_ppo_sched_begin(const hwy_ppo_sched_plan* plan, void* table, void* stream);
int hwy_ppo_sched_step(const hwy_ppo_sched_plan* plan, const void* table, int slot, void* stream);
int hwy_ppo_sched_advance(const hwy_ppo_sched_plan* plan, void* table, int slots, void* stream);

/* ---- The scheduled update with a per-learner KL stop: hwy_ppo_sched_step with a control block
 * beside the table.  Learner y has kl_on[y] (0 / 1) and kl_limit[y].  In a slot in which y is
 * active, after the weight-gradient launch has written the step's metrics row, kl = column 5 of
 * that row exactly as stored; y TRIPS iff kl_on && !(kl <= kl_limit) (a NaN trips).  The tripping
 * step is discarded: its slice-sum and Adam launches write nothing of y (params, adam_m, adam_v,
 * tile image), and counters[0] ends as if the step had not run.  From then on y sits every slot
 * of the update out, untouched, as a learner whose epochs are done does.  After an update that
 * applied k steps of y: counters[0] += k, counters[1] += k + 1 (the tripping row, whose six
 * metrics are valid; later rows are not written); without a trip, and always with kl_on == 0, y
 * is bit for bit what hwy_ppo_sched_step makes it.  The trip state is cleared by
 * hwy_ppo_sched_ctl_begin only: it survives graph replays and hwy_ppo_sched_advance.
 *
 * Control block (hwy_ppo_sched_ctl_bytes(G) bytes of device memory, sections 256-byte aligned):
 *   byte 0                           G x { int32 kl_on; float kl_limit; }
 *   hwy_ppo_sched_ctl_stopped_offset(G) = round_up_256(8 G)
 *                                    G x int32 stopped_at: the slot that tripped, -1 if none
 *   + round_up_256(4 G)              G x int32, the library's own copy of stopped_at
 * stopped_at[y] is written by one thread's ordinary store in the tripping slot's slice-sum launch
 * and is stable once the update's work on the stream is done: the host reads it with the copy it
 * makes of the metrics anyway, no further synchronisation.  No step launch reads a control word
 * that the same launch writes (a word written in launch n is read by launches after n only).
 *
 * hwy_ppo_sched_ctl_prepare is synchronous (host arrays; it waits for `stream`) and not
 * capturable; begin (= hwy_ppo_sched_begin + clearing the trip state) and step are asynchronous,
 * allocate nothing and are hipGraph-capturable; hwy_ppo_sched_advance serves both step calls.
 *
 * hwy_ppo_sched_set_lr: from then on (stream order) the Adam launches of hwy_ppo_sched_step and
 * hwy_ppo_sched_ctl_step on `table` use lr_dev[y] (device floats) as learner y's learning rate --
 * an update after it is bit for bit one whose table was prepared with args.lr = that value.
 * Asynchronous, capturable; issue it between whole slots.
 * -1 bad arguments (before any device call), -2 HIP error. */
int64_t hwy_ppo_sched_ctl_bytes(int G);
int64_t hwy_ppo_sched_ctl_stopped_offset(int G);
int hwy_ppo_sched_ctl_prepare(const hwy_ppo_sched_plan* plan, const float* kl_limit /*[G]*/,
                              const int32_t* kl_on /*[G]*/, void* ctl, void* stream);
int hwy_ppo_sched_ctl_begin(const hwy_ppo_sched_plan* plan, void* table, void* ctl, void* stream);
int hwy_ppo_sched_ctl_step(const hwy_ppo_sched_plan* plan, const void* table, void* ctl, int slot,
                           void* stream);
int hwy_ppo_sched_set_lr(const hwy_ppo_sched_plan* plan, void* table, const float* lr_dev /*[G]*/,
                         void* stream);

/* ---- Input gradients: what the policy's outputs depend on in its observation.  For B rows of
 * states and K cotangents per row (1 <= K <= 4)
 *   dstates[k][b][:] = sum_o cot[k][b][o] * d out_o(states[b]) / d states[b],
 *   out = (mean_0, mean_1, value):
 * mean is the pre-tanh actor mean (hwy_ppo_act's pre_tanh with noise == NULL), value the critic's
 * output; log_std does not enter.  The forward is hwy_ppo_act's without a tile image (16-row
 * tiles; past S = 256 the chunked first layer), run once per tile; mean / value, when given, are
 * bit for bit hwy_ppo_act(noise = NULL, tiles = NULL)'s pre_tanh / value on the same inputs.  Per
 * cotangent the backward is
 *   dac = relu'(a1 | c1) * (cot_0 wa2[0] + cot_1 wa2[1] | cot_v wc2)
 *   dh2 = relu'(h2) * (dac [Wa1; Wc1])    dh1 = relu'(h1) * (dh2 W2)    dS = dh1 W1
 * with relu' = 1 iff the kernel's own fp32 pre-activation is > 0 (torch's convention, 0 at 0); the
 * products are fp32 MFMA over params read in place (no tile image is used or needed).
 * Exact by construction: a row whose cotangent is all zero gets a zero dstates row; a state column
 * whose W1 column is all zero gets zeros; cotangent k of a K-cotangent call has the bits of a
 * one-cotangent call; a row's results do not depend on B or on the other rows.  Nothing outside
 * dstates, mean, value and relu_bits is written.  Needs S % 4 == 0, 0 < S <= 1024,
 * H in {64, 128, ..., 512}, A == 2.  Asynchronous, allocates nothing, hipGraph-capturable.
 * -1 bad arguments (a NULL states / params / cot / dstates, K outside 1..4, dims outside the range),
 * before any device call; -2 HIP error. */
typedef struct hwy_ppo_input_grad_args {
  hwy_ppo_dims dims;
  const float* states;    /* [B][S] contiguous */
  const float* params;    /* flat, hwy_ppo_param_layout order */
  int32_t K;              /* 1..4 */
  const float* cot;       /* [K][B][3] device: weights of (mean_0, mean_1, value) per row */
  float* dstates;         /* [K][B][S] */
  float* mean;            /* nullable [B][2] */
  float* value;           /* nullable [B] */
  uint32_t* relu_bits;    /* nullable [B][4][H/32]: layers z1, z2, za, zc; bit (c % 32) of word
                             c / 32 set iff the kernel's own pre-activation of unit c is > 0 */
} hwy_ppo_input_grad_args;
int hwy_ppo_input_grad(const hwy_ppo_input_grad_args* a, void* stream);
int hwy_ppo_input_grad_args_size(void); /* sizeof(hwy_ppo_input_grad_args), for a binding's check */

/* Build flags of this library: bit 0 = development knobs compiled in (HWY_DEV_KNOBS: the
 * HWY_WG_BAL / HWY_ROWS_RT / HWY_WG_FILL environment variables are read), bit 1 = section clocks
 * (HWY_SECTION_PROFILE).  A product build returns 0 and reads no environment variable. */
int hwy_ppo_build_flags(void);

#ifdef __cplusplus
}
#endif
#endif /* HWY_PPO_H_ */
