/*
 * hwy.h -- C ABI of libhwy.so, the MI355X-native vectorised highway-v0 step.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json:north_star.
 * Every entry point below replaces one reference interface (reference = DhruvDh/highway-rope-ppo,
 * paths relative to its repo root; highway-env 1.10.1 is the third-party package the reference
 * calls, pinned at uv.lock:163-178 and NOT vendored):
 *
 *   hwy_create / hwy_destroy  <- gym.make("highway-v0", config=cfg)      experiments/wrappers.py:80
 *                                env.close()                             experiments/runner.py:139-142
 *   hwy_reset                 <- env.reset(seed=exp_seed + episode_num)  training/routine.py:127
 *                                env.reset(seed=exp_seed + 1000 + ep)    training/routine.py:18
 *   hwy_step                  <- env.step(action)                        training/routine.py:24,134
 *                                (AbstractEnv.step/_simulate, HighwayEnv._reward/_is_terminated/
 *                                 _is_truncated, KinematicObservation.observe [highway-env 1.10.1])
 *                                + the PE wrapper's .observation() fused in (pe_kind != 0)
 *   hwy_step_with_info        <- the info dict of env.step: AbstractEnv._info (speed, crashed,
 *                                action) with HighwayEnv._rewards' four terms as "rewards"
 *                                [highway-env 1.10.1], plus per-episode sums of them
 *   hwy_cut_episodes          <- the collection loop's cut at steps_per_update
 *                                                                        training/routine.py:125-132,153-156
 *   hwy_set_pe_table          <- RankEmbedWrapper.__init__ table        experiments/rank_embed.py:21-22
 *                                DistanceEmbedWrapper freqs               experiments/dist_embed.py:48-52
 *                                RotaryEmbedWrapper inv_freq              experiments/rope_embed.py:36-39
 *   hwy_obs_pe                <- RotaryEmbedWrapper.observation          experiments/rope_embed.py:64-74
 *                                RotaryEmbedWrapper._apply_rope          experiments/rope_embed.py:44-62
 *                                DistanceEmbedWrapper.observation        experiments/dist_embed.py:76-96
 *                                RankEmbedWrapper.observation            experiments/rank_embed.py:45-51
 *   hwy_gae                   <- PPOMemory.compute_advantages            ppo/agent.py:126-138
 *   hwy_set_seed_groups       <- one gym.make per experiment of a sweep  experiments/runner.py:73-78
 *   hwy_step_group            <- env.step of every cell of a sweep batch (one launch)
 *                                (main.py:188-242 fans the seeds out as separate processes; here
 *                                 a cell's seeds share one handle, each with its own schedule)
 *   hwy_step_group_info       <- the same, every cell's step with its info outputs
 *   hwy_step_with_final       <- the terminal observation of an autoresetting vector env
 *                                (gymnasium's info["final_observation"]; the reference steps one
 *                                 env and resets it by hand, so it holds the row itself,
 *                                 training/routine.py:134-150)
 *   hwy_step_group_final      <- the same through the grouped launch's tables
 *   hwy_gae_boot              <- PPOMemory.compute_advantages with the value of the final
 *                                observation at a time limit instead of 0 (the reference books
 *                                truncation as terminal, training/routine.py:135; opt-in)
 *   hwy_render                <- env.render() of a render_mode="rgb_array" env  visualize.py:146
 *                                (this project's own frame rule, not pygame's pixels)
 *   hwy_observe               <- env.unwrapped.observation_type.observe() on the current road, under
 *                                either "order", plus the row -> vehicle assignment it drops
 *   hwy_sense                 <- nothing upstream: observation_type.observe() of the vehicles a sensor
 *                                on the ego perceives (range, line of sight, dropout, noise)
 *   hwy_traffic               <- env.unwrapped.road.neighbour_vehicles(v) for every vehicle, and the
 *                                gap / time-to-collision / headway a driving study derives from it
 *   hwy_lookahead             <- copy.deepcopy(env) then env.step(a), repeated, for K action sequences
 *   hwy_grid                  <- OccupancyGridObservation.observe() [highway-env 1.10.1] of a
 *                                Kinematics env's road (this project's own rule, not upstream's bits)
 *   hwy_lidar                 <- LidarObservation.observe() [highway-env 1.10.1] of a Kinematics
 *                                env's road (this project's own rule, not upstream's trace())
 *
 * Conventions
 *   - Plain pointers and sizes only; device pointers are HIP device pointers (e.g. torch
 *     tensor.data_ptr()), `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - All compute calls are stream-ordered and asynchronous; none allocates or synchronises,
 *     so they can be captured into a hipGraph.
 *   - Return value: 0 on success, <0 on error; hwy_last_error() gives a thread-local message.
 *     HWY_EINVAL errors are configuration errors (the Python layer raises ValueError, as the
 *     reference's make_env / wrapper constructors do).
 *   - A handle is not thread-safe; use one handle per GPU rank.
 */
#ifndef HWY_H_
#define HWY_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HWY_ABI_VERSION 1

#define HWY_MAX_VEHICLES 64 /* simulated vehicles per env incl. ego (one wavefront lane each) */
#define HWY_MAX_FEATURES 8  /* observation features per row */
#define HWY_MAX_OBS_ROWS 64 /* observed rows N */
#define HWY_MAX_FOUT 64     /* features per row after the PE wrapper */
#define HWY_MAX_PE_TABLE 4096

#define HWY_OK 0
#define HWY_EINVAL (-1)
#define HWY_EDEVICE (-2)
#define HWY_ENOMEM (-3)

/* Kinematics observation features (KinematicObservation FEATURES / Vehicle.to_dict keys). */
enum hwy_feature {
  HWY_FEAT_PRESENCE = 0,
  HWY_FEAT_X = 1,
  HWY_FEAT_Y = 2,
  HWY_FEAT_VX = 3,
  HWY_FEAT_VY = 4,
  HWY_FEAT_COS_H = 5,
  HWY_FEAT_SIN_H = 6,
  HWY_FEAT_HEADING = 7
};

enum hwy_order { HWY_ORDER_SORTED = 0, HWY_ORDER_SHUFFLED = 1 };

/* Observation wrapper fused into the step (experiments/wrappers.py:91-104). */
enum hwy_pe_kind {
  HWY_PE_NONE = 0,
  HWY_PE_RANK = 1,  /* RankEmbedWrapper */
  HWY_PE_DIST = 2,  /* DistanceEmbedWrapper(use_euclidean=True) */
  HWY_PE_ROPE = 3,  /* RotaryEmbedWrapper */
  HWY_PE_DIST1 = 4  /* DistanceEmbedWrapper(use_euclidean=False): |x_i - x_ego| */
};

/* Mirrors HIGHWAY_CONFIG (config/base_config.py:5-39) after make_env's deep merge and
 * order resolution (experiments/wrappers.py:33-57). */
typedef struct hwy_config {
  int32_t num_envs;        /* E: envs owned by this handle */
  int32_t lanes_count;     /* "lanes_count" (4) */
  int32_t vehicles_count;  /* "vehicles_count" (50 traffic cars; +1 ego simulated) */
  int32_t obs_vehicles;    /* observation "vehicles_count" N (15) */
  int32_t n_features;      /* F */
  int32_t feature_ids[HWY_MAX_FEATURES];      /* enum hwy_feature, row order */
  int32_t has_range[HWY_MAX_FEATURES];        /* feature has a features_range entry */
  float features_range[HWY_MAX_FEATURES][2];  /* [lo, hi] per feature */
  int32_t order;           /* enum hwy_order */
  int32_t absolute;        /* "absolute" */
  int32_t normalize;       /* "normalize" */
  int32_t clip;            /* KinematicObservation clip (default True) */
  int32_t see_behind;      /* KinematicObservation see_behind (default False) */
  int32_t sim_freq;        /* "simulation_frequency" (15) */
  int32_t policy_freq;     /* "policy_frequency" (1) */
  int32_t max_steps;       /* truncation horizon in policy steps (horizon) */
  int32_t initial_lane_id; /* "initial_lane_id" (-1 = random) */
  float vehicles_density;  /* "vehicles_density" (2) */
  float ego_spacing;       /* "ego_spacing" (2) */
  float speed_limit;       /* straight_road_network speed_limit (30) */
  float collision_reward, right_lane_reward, high_speed_reward, lane_change_reward;
  float on_road_reward;    /* config.get("on_road_reward", 0) */
  float reward_speed_range[2];
  int32_t normalize_reward; /* "normalize_reward" (True) */
  int32_t offroad_terminal; /* "offroad_terminal" (False) */
  /* fused observation wrapper */
  int32_t pe_kind;          /* enum hwy_pe_kind */
  int32_t d_embed;          /* rank / dist: appended width d; rope: rotate_dim */
  int32_t ego_idx;          /* wrapper ego_idx (0) */
  float pe_max_dist;        /* utils/defaults.py:max_dist() (100) */
  /* episode schedule: seed(env e, episode k) = seed_base + env_offset + e + 1 + seed_stride*k,
   * i.e. training/routine.py:127's exp_seed + episode_num for E = 1. */
  int32_t autoreset;        /* reset finished envs inside hwy_step */
  int32_t env_offset;       /* global index of this handle's env 0 (rank * E) */
  int64_t seed_base;
  int64_t seed_stride;      /* global env count */
} hwy_config;

typedef struct hwy_handle hwy_handle;

/* Per-env state: uint32 words laid out [HWY_NFIELDS][num_envs][HWY_MAX_VEHICLES] (field-major
 * SoA; one wavefront reads 256 contiguous bytes per field). Lane v of an env is vehicle v in
 * road.vehicles order (v = 0 is the ego). Float fields hold IEEE binary32 bits. */
enum hwy_field {
  HWY_F_X = 0, HWY_F_Y, HWY_F_HEADING, HWY_F_SPEED,
  HWY_F_TSPEED,  /* IDM target_speed */
  HWY_F_DELTA,   /* IDM DELTA exponent (randomize_behavior) */
  HWY_F_TIMER,   /* MOBIL lane-change timer */
  HWY_F_IMPX, HWY_F_IMPY, /* pending collision impact */
  HWY_F_LANE,    /* int: closest lane id */
  HWY_F_TLANE,   /* int: target lane id */
  HWY_F_FLAGS,   /* int: bit0 crashed, bit1 impact pending, bit2 present, bits 8-13 the
                    vehicle's position in the road order (x ascending, index descending) of the
                    stored positions -- a hint the step validates before use */
  HWY_F_ENV,     /* per-env words, see enum hwy_env_word */
  HWY_NFIELDS
};
enum hwy_env_word {
  HWY_E_STEP = 0,    /* policy steps taken this episode */
  HWY_E_EPISODE,     /* per-env episode counter k */
  HWY_E_SEED_LO, HWY_E_SEED_HI, /* seed of the current episode */
  HWY_E_EGO_ACC, HWY_E_EGO_STEER, /* float: ego action dict (persists across frames) */
  HWY_E_RETURN,      /* float: running episode return */
  HWY_E_NWORDS
};
#define HWY_FLAG_CRASHED 1u
#define HWY_FLAG_IMPACT 2u
#define HWY_FLAG_PRESENT 4u
#define HWY_FLAG_ORDER_SHIFT 8u
#define HWY_FLAG_ORDER_MASK (63u << HWY_FLAG_ORDER_SHIFT)

int hwy_abi_version(void);
/* sizeof(hwy_config) as compiled into the library (binding layout check). */
int hwy_config_size(void);
const char* hwy_last_error(void);

/* Validates cfg and allocates the device state for cfg->num_envs envs on `device`. */
int hwy_create(const hwy_config* cfg, int device, hwy_handle** out);
void hwy_destroy(hwy_handle* h);
/* Feature count per observation row after the fused wrapper (F or F + d). */
int hwy_obs_features(const hwy_handle* h);

/* Host table for the fused wrapper: rank -> tanh(W) [N*d]; dist -> freqs [d/2];
 * rope -> inv_freq [rotate_dim/2]; with experiment groups (hwy_set_seed_groups) also
 * n_groups RankPE tables [n_groups*N*d], one per group. Synchronous (setup time only). */
int hwy_set_pe_table(hwy_handle* h, const float* table_host, int n);

/* Change the episode seed schedule (seed_base, env_offset, seed_stride) of an existing handle:
 * training/routine.py re-seeds every episode from exp_seed (routine.py:127) and every evaluation
 * from exp_seed + 1000 (routine.py:18).  Takes effect for the next reset / autoreset. */
int hwy_set_seed_schedule(hwy_handle* h, int64_t seed_base, int32_t env_offset, int64_t seed_stride);

/* Experiment groups (a sweep's seeds batched into one handle; experiments/sweep.py): the E envs
 * form E / envs_per_group groups of consecutive envs, group g an experiment of its own with
 * seed(env g*envs_per_group + l, episode k) = seed_bases[g] + env_offset + l + 1 + seed_stride*k
 * (set seed_stride = envs_per_group for the solo schedule of each group: the same seeds, so each
 * group's envs step bit for bit as a solo handle of envs_per_group envs would).  seed_bases
 * (host, [E / envs_per_group]) is copied; n_groups = 0 turns grouping off.  With a fused RankPE,
 * hwy_set_pe_table may then take n_groups tables back to back (group g reads table g).  A later
 * call with the same n_groups and envs_per_group keeps them (group g still reads table g); any
 * other call, n_groups = 0 included, leaves them without meaning: every reset, step, cut and
 * prepare then returns HWY_EINVAL until hwy_set_pe_table is called again.
 * Synchronous (setup time only). */
int hwy_set_seed_groups(hwy_handle* h, const int64_t* seed_bases, int n_groups, int envs_per_group);

/* Reset envs whose mask byte is nonzero (mask NULL = all) with the given per-env seeds
 * (seeds NULL = the autoreset schedule with k = 0). Writes obs [E, N, F_out] for reset envs. */
int hwy_reset(hwy_handle* h, const uint64_t* seeds, const uint8_t* mask, float* obs, void* stream);

/* One policy step (sim_freq/policy_freq frames) for all E envs.
 *   actions [E,2] f32 in; obs [E,N,F_out], reward [E] f32, terminated/truncated [E] u8 out.
 *   ep_return / ep_length (nullable) receive the finished episode's return / length where
 *   terminated|truncated (0 elsewhere). With cfg.autoreset, finished envs are reset and obs
 *   holds the first observation of the next episode. */
int hwy_step(hwy_handle* h, const float* actions, float* obs, float* reward, uint8_t* terminated,
             uint8_t* truncated, float* ep_return, int32_t* ep_length, void* stream);

/* ---- Step with info: hwy_step plus the ego's per-step info (upstream's AbstractEnv._info and
 * HighwayEnv._rewards) and running per-episode sums.  The env computes exactly what hwy_step
 * computes (the same kernel body; the outputs below are extra stores).  All pointers are device
 * pointers and nullable; values are the ego's after the step's frames, before any autoreset:
 *   speed [E] f32      Vehicle.speed
 *   crashed [E] u8     Vehicle.crashed
 *   lane [E] i32       the ego's lane id (lane_index[2])
 *   rewards [E,4] f32  collision_reward, right_lane_reward, high_speed_reward, on_road_reward of
 *                      HighwayEnv._rewards: the unweighted terms, exactly as they enter the reward
 *   acc [E,HWY_INFO_NACC] f32, in/out, caller-owned: the current episode's running sums --
 *                      [0] sum of speed, [1..4] sums of the four terms, [5] steps on which the
 *                      lane id after the step differs from the one before it, [6], [7] reserved
 *                      (written 0).  Each step does acc = acc + value in float32, as ep_return.
 *                      An env whose step count is 0 on entry (just reset, autoreset or cut) starts
 *                      from zero, not from the buffer, so the buffer needs no clearing.  After
 *                      hwy_cut_episodes the rows of the cut envs hold their partial sums.
 *   ep_stats [E,HWY_INFO_NACC] f32  where terminated|truncated: the finished episode's sums with
 *                      [6] = the ego's crashed flag; all 0 elsewhere (as ep_return).  Needs acc.
 * Returns HWY_EINVAL for a NULL handle, NULL info, or ep_stats without acc. */
#define HWY_INFO_NACC 8
typedef struct hwy_step_info {
  float* speed;
  uint8_t* crashed;
  int32_t* lane;
  float* rewards;
  float* acc;
  float* ep_stats;
} hwy_step_info;
/* sizeof(hwy_step_info) as compiled into the library (binding layout check). */
int hwy_step_info_size(void);
int hwy_step_with_info(hwy_handle* h, const float* actions, float* obs, float* reward,
                       uint8_t* terminated, uint8_t* truncated, float* ep_return,
                       int32_t* ep_length, const hwy_step_info* info, void* stream);

/* End every running episode and start the next one of the schedule (the reference's collection
 * loop, training/routine.py:125-132, 153-156).  For each env whose episode has taken >= 1 policy
 * step: cut[e] = 1, ep_return[e] / ep_length[e] = its running return / steps so far, then exactly
 * what hwy_step's autoreset does at a truncation: episode k -> k + 1, seed = the schedule's seed
 * for (e, k + 1) (seed groups included), reset, first observation written to obs row e.
 * An env at step 0 (it finished on its last step and was autoreset, or was just reset) is not
 * touched: cut[e] = 0, ep_return[e] = 0, ep_length[e] = 0, its obs row is NOT written, its
 * state words stay.  obs [E,N,F_out]; ep_return / ep_length / cut nullable.  Asynchronous,
 * allocates nothing, hipGraph-capturable.  Meant for cfg.autoreset handles, where a finished env
 * is back at step 0.  With autoreset off the launch works the same way, but an env that hwy_step
 * has just reported terminated / truncated still holds its step count: the cut would book that
 * episode a second time (cut = 1 and the return hwy_step already gave) before restarting it, so
 * such a caller masks those envs out of what it reads back. */
int hwy_cut_episodes(hwy_handle* h, float* obs, float* ep_return, int32_t* ep_length,
                     uint8_t* cut, void* stream);

/* ---- Grouped step: n handles (the cells of a sweep batch, each one experiment group's handle;
 * ppo/group.py GroupBatch) stepped in ONE launch instead of n.  Workgroup (x, y) runs hwy_step's
 * workgroup x for handle y, reading that handle's launch parameters from a device table; each
 * env computes exactly what hwy_step on its own handle computes (the same kernel body).  Handles
 * may differ in env count, observation width and fused wrapper; one launch takes the register
 * budget of the handles' total env count.  hwy_step_group_prepare builds the table from the
 * handles as they are now and the per-handle buffers io[i] (hwy_step's arguments); it is
 * synchronous (waits for `stream`) and must be redone after any handle's configuration changes
 * (seed schedule, groups, PE table).  hwy_step_group is asynchronous and hipGraph-capturable. */
typedef struct hwy_step_io {
  const float* actions;
  float* obs;
  float* reward;
  uint8_t* terminated;
  uint8_t* truncated;
  float* ep_return;  /* nullable */
  int32_t* ep_length; /* nullable */
} hwy_step_io;
typedef struct hwy_step_group_plan {
  int32_t n, blocks, big; /* handles; workgroups per handle (the largest); register budget */
} hwy_step_group_plan;
int64_t hwy_step_group_table_bytes(int n);
int hwy_step_group_prepare(hwy_handle* const* handles, const hwy_step_io* io, int n, void* table,
                           hwy_step_group_plan* plan, void* stream);
int hwy_step_group(const hwy_step_group_plan* plan, const void* table, void* stream);
/* The grouped step with info: info[i] is handle i's hwy_step_info (its pointers nullable as for
 * hwy_step_with_info), kept in a second device table of hwy_step_group_info_table_bytes(n) bytes
 * beside the step table (hwy_step_group_table_bytes(n), which hwy_step_group can launch too).
 * The same rules as above: prepare is synchronous, the launch asynchronous and capturable. */
int64_t hwy_step_group_info_table_bytes(int n);
int hwy_step_group_info_prepare(hwy_handle* const* handles, const hwy_step_io* io,
                                const hwy_step_info* info, int n, void* table, void* info_table,
                                hwy_step_group_plan* plan, void* stream);
int hwy_step_group_info(const hwy_step_group_plan* plan, const void* table, const void* info_table,
                        void* stream);

/* ---- Step with the terminal observation: hwy_step_with_info (info nullable here: NULL = no info
 * outputs) that also writes, for every env whose episode finished in this step (terminated or
 * truncated), the last observation of that episode to final_obs [E][N][F_out] -- what a handle
 * with autoreset off would have written to obs: the pre-reset vehicles, the finished episode's
 * step count and seed (the shuffled order depends on both) and the same PE table.  Rows of envs
 * that are not done are not written.  With autoreset off the row equals the obs row.  The env
 * computes exactly what hwy_step computes.  HWY_EINVAL for a NULL handle, a NULL final_obs,
 * final_obs == obs, or info->ep_stats without info->acc. */
int hwy_step_with_final(hwy_handle* h, const float* actions, float* obs, float* reward,
                        uint8_t* terminated, uint8_t* truncated, float* ep_return,
                        int32_t* ep_length, const hwy_step_info* info /*nullable*/,
                        float* final_obs, void* stream);
/* The grouped form: info (nullable; else [n], each as above) and final_obs [n] live in a second
 * device table of hwy_step_group_final_table_bytes(n) bytes beside the step table
 * (hwy_step_group's format).  Prepare is synchronous, the launch asynchronous and capturable. */
int64_t hwy_step_group_final_table_bytes(int n);
int hwy_step_group_final_prepare(hwy_handle* const* handles, const hwy_step_io* io,
                                 const hwy_step_info* info /*nullable*/,
                                 float* const* final_obs /*[n]*/, int n, void* table,
                                 void* final_table, hwy_step_group_plan* plan, void* stream);
int hwy_step_group_final(const hwy_step_group_plan* plan, const void* table,
                         const void* final_table, void* stream);

/* Copy the packed state [HWY_NFIELDS][E][HWY_MAX_VEHICLES] u32 to / from device memory. */
int hwy_export_state(hwy_handle* h, uint32_t* dst, void* stream);
int hwy_import_state(hwy_handle* h, const uint32_t* src, void* stream);

/* ---- Frames of the env states (the reference's render_mode="rgb_array" envs, visualize.py and
 * training/routine.py:visualize_agent; upstream draws with pygame, whose pixels are NOT
 * reproduced: the frame is defined by the rule below, with upstream's view geometry -- 600x150,
 * 5.5 px/m, the ego at 0.3 / 0.5 of the frame -- as the Python layer's defaults).
 *
 * Frame i shows env e = env_ids[i] (e = i when env_ids is NULL), drawn from the state words as
 * they stand: after an autoreset that is the new episode, as the obs row the step wrote.  An
 * env_ids entry outside 0..E-1 gives an all-background frame (the state is never indexed with it).
 * All geometry is relative to the ego (vehicle 0, at (xe, ye)) and computed in binary32.
 *
 * Pixel centre of row r, column c, in metres from the ego (x right along the road, y down toward
 * higher lane ids):
 *   px = ((c + 0.5) - centering[0] * width)  / scaling
 *   py = ((r + 0.5) - centering[1] * height) / scaling
 * Layers, the later one wins:
 *   1. background
 *   2. road surface where -xe <= px <= 10000 - xe (ROAD_LENGTH) and y_0 <= py < y_L, with
 *      y_k = (4k - 2) - ye for k = 0..L, L = lanes_count
 *   3. lane lines, inside the road's x extent only, where |py - y_k| <= LINE_HALF; k = 0 and
 *      k = L solid, 0 < k < L dashed and anchored to the world: with ph = xe - 8 floor(xe / 8)
 *      (exact in binary32) and u = px + ph, a dash is drawn where u - 8 floor(u / 8) < DASH_ON
 *   4. vehicles 1..63 in ascending index (a later one paints over an earlier one), each iff its
 *      flags carry HWY_FLAG_PRESENT: with dx = px - (x_v - xe), dy = py - (y_v - ye) (the two
 *      differences in parentheses taken first) and (sh, ch) = hm_sincosf(heading_v), the pixel
 *      is covered iff |dx ch + dy sh| <= 2.5 and |dy ch - dx sh| <= 1.0 (VEH_LENGTH / 2,
 *      VEH_WIDTH / 2)
 *   5. the ego, by the same test, on top
 * A comparison with a NaN is false: a vehicle at a non-finite position is not drawn, and a frame
 * whose ego is non-finite is all background.
 *
 *   constant      value            meaning
 *   BACKGROUND    ( 60,  60,  60)  layer 1
 *   ROAD          (100, 100, 100)  layer 2
 *   LINE          (255, 255, 255)  layer 3
 *   VEHICLE       (100, 200, 255)  layer 4
 *   EGO           ( 50, 200,   0)  layer 5
 *   CRASHED       (255, 100, 100)  any vehicle, the ego included, with HWY_FLAG_CRASHED
 *   HOT           (255, 220,   0)  what `shade` tints toward
 *   LINE_HALF     0.15 m           half width of a lane line
 *   DASH_ON       3 m of every 8   drawn part of a dashed line
 * (the palette, LINE_HALF and DASH_ON are this project's constants, not upstream's).
 *
 * shade (nullable; device float [E][64], vehicle order) tints vehicle v of env e toward HOT in
 * integer arithmetic: s8 = (int)(clamp(s, 0, 1) * 256), NaN giving 0, and per channel
 * (base (256 - s8) + HOT s8 + 128) >> 8 -- the base colour at s = 0 and HOT at s = 1, exactly.
 * channels == 1 writes the luma (77 R + 150 G + 29 B + 128) >> 8 of the RGB pixel.
 *
 * hwy_render is asynchronous, allocates nothing, is hipGraph-capturable, reads the state and
 * writes nothing but `frames`.  Bad arguments return HWY_EINVAL before any device call. */
typedef struct hwy_render_args {
  int32_t width, height;   /* pixels, each 1..4096 */
  int32_t channels;        /* 3 = RGB, 1 = luma */
  int32_t n;               /* frames, 1..2^22 */
  float scaling;           /* pixels per metre: finite, > 0 */
  float centering[2];      /* finite */
  const int32_t* env_ids;  /* device [n] in 0..E-1, nullable (then n <= E) */
  const float* shade;      /* device [E][64], nullable */
  uint8_t* frames;         /* device [n][height][width][channels], 16-byte aligned */
} hwy_render_args;
/* sizeof(hwy_render_args) as compiled into the library (binding layout check). */
int hwy_render_args_size(void);
/* n * height * width * channels, or -1 for arguments hwy_render refuses (every check that needs
 * no handle); pure, no device call. */
int64_t hwy_render_frame_bytes(const hwy_render_args* a);
int hwy_render(hwy_handle* h, const hwy_render_args* a, void* stream);

/* ---- Re-observe the env states: the observation as a function of the stored state, the vehicle
 * each row shows, the other row order, and per-row values scattered to the vehicles.
 *
 * hwy_observe observes all E envs from the state words as they stand, with the step's own
 * observation code (the same function hwy_step / hwy_reset / hwy_cut_episodes run on exactly what
 * they then store: the vehicles' x, y, heading, speed and flags and the env's step and seed words;
 * sin / cos are hm_sincosf of the stored heading).
 *
 *   order -1, or the handle's own order: obs [E][N][F_out] is bit for bit the row the last
 *     hwy_step* / hwy_reset / hwy_cut_episodes wrote for that env -- after an autoreset the new
 *     episode's first observation -- for every fused wrapper and for seed groups with their
 *     per-group RankPE tables.
 *   the other order: obs is what that same call would have written had the handle's `order` been
 *     the other one, everything else as the handle's config, the fused wrapper included: RankPE
 *     appends table[row position], the distance wrappers see the reordered rows.  `shuffled` is
 *     the step's permutation: Philox over (slot, step word, seed words), N - 1 slots, empty slots
 *     shuffled along with the full ones, identity for N <= 2.
 *   row_vehicle [E][N] i32: the vehicle index (0..63) shown in row r, -1 for an empty (all-zero)
 *     row; row 0 is always 0 (the ego).  Non-negative entries of an env are distinct.
 *   row_values [E][N] f32 in, veh_values [E][64] f32 out (hwy_render's `shade` layout), both or
 *     neither: veh_values[e][row_vehicle[e][r]] = row_values[e][r], bits copied, for every row
 *     with a vehicle; every other entry of the 64 is written +0.0.
 *
 * All pointers are device pointers and nullable, but at least one output must be given.
 * hwy_observe is asynchronous, allocates nothing, is hipGraph-capturable, reads the state and
 * writes nothing but the outputs it was given.  It returns HWY_EINVAL before any device call for
 * a NULL handle or NULL args, an order outside {-1, HWY_ORDER_SORTED, HWY_ORDER_SHUFFLED}, all of
 * obs / row_vehicle / veh_values NULL, row_values without veh_values or the reverse, and a handle
 * whose per-group PE tables are without meaning (hwy_set_seed_groups). */
typedef struct hwy_observe_args {
  int32_t order;            /* -1: the handle's own; else enum hwy_order */
  float* obs;               /* device [E][N][F_out], nullable */
  int32_t* row_vehicle;     /* device [E][N], nullable */
  const float* row_values;  /* device [E][N], nullable; needs veh_values */
  float* veh_values;        /* device [E][64], nullable; needs row_values */
} hwy_observe_args;
/* sizeof(hwy_observe_args) as compiled into the library (binding layout check). */
int hwy_observe_args_size(void);
/* HWY_OK, or HWY_EINVAL for arguments hwy_observe refuses (every check that needs no handle);
 * pure, no device call. */
int hwy_observe_check(const hwy_observe_args* a);
int hwy_observe(hwy_handle* h, const hwy_observe_args* a, void* stream);

/* ---- Traffic measures of the env states: who drives in front of and behind whom, the
 * bumper-to-bumper gap, the time-to-collision (TTC) and the time headway (THW), an ego row, and a
 * running per-episode reduction of the ego's.
 *
 * hwy_traffic reads the state words as they stand (x, y, heading, speed, the lane word and the
 * flags) with the step's own neighbour search, so "front" is the vehicle IDM would brake for.
 *
 * Neighbour rule (Road.neighbour_vehicles).  The candidates for vehicle i on lane c are the other
 * present vehicles k with |y_k - 4c| <= 3 (one float32 subtraction) and -5 <= x_k < 10005.
 *   front = the nearest candidate with x_i <= x_k; among equal x the last in vehicle order
 *   rear  = the nearest candidate with x_k < x_i;  among equal x the first in vehicle order
 * A vehicle's own lane is its stored HWY_F_LANE word (no neighbour on a lane outside the road).
 *
 * Per-vehicle outputs, [E][64] in hwy_render's `shade` layout, vx = speed * cos(heading) with
 * hm_sincosf's cosine:
 *   front, rear (i32)  vehicle index on the own lane, -1 for none
 *   gap     (x_f - x_i) - 5.0f, the two float32 subtractions in that order; +inf without a front
 *   closing vx_i - vx_f; 0 without a front
 *   ttc     0 where gap <= 0, else gap / closing where closing > 0, else +inf
 *   thw     0 where gap <= 0, else gap / vx_i where vx_i > 0, else +inf
 *   risk    1 - ttc / risk_horizon where ttc < risk_horizon, else 0 (in [0, 1]: usable as
 *           hwy_render's shade as it is)
 * Absent slots and lanes >= vehicles_count + 1 are written the "none" values: front = rear = -1,
 * gap = ttc = thw = +inf, closing = risk = 0.  No entry is left unwritten.
 *
 * ego [E][HWY_TRAFFIC_NEGO] f32, of vehicle 0 (x_e, y_e, vx_e, lane word ln):
 *   0-3   front gap, closing, ttc, thw (vehicle 0's entries above)
 *   4     rear gap (x_e - x_r) - 5.0f, +inf without a rear
 *   5     rear closing vx_r - vx_e, 0 without a rear
 *   6     rear ttc, from slots 4 and 5 by the front ttc's rule
 *   7-10  front gap and rear gap on lane ln - 1, then on lane ln + 1: the same expressions towards
 *         that lane's front / rear of the ego; +inf where the lane or the vehicle does not exist.
 *         They may be negative (down to -5 in front) when a car is alongside.
 *   11    the least centre distance to any other present vehicle: sqrt of the least
 *         dx*dx + dy*dy (two products and a sum, no fused multiply-add); +inf with none
 *   12    the count of other present vehicles with 0 <= x_k - x_e <= near_range
 *   13    y_e - 4 ln
 *   14    vx_e
 *   15    risk of the ego
 *
 * acc [E][HWY_TRAFFIC_NACC] f32, in/out, caller-owned, zero-filled once by the caller: the running
 * reduction of the ego's measures over the states of the current episode,
 *   0 states counted n        1 min front ttc      2 min front thw     3 min front gap
 *   4 min centre distance     5 states with ttc < ttc_thresh           6 states with thw <
 *   thw_thresh                7 states with a front vehicle
 * restart[0..2]: up to three nullable [E] u8 masks, OR-ed (meant for a step's terminated and
 * truncated and hwy_cut_episodes' cut).  For a marked env ep_stats[e] ([E][8], nullable, needs
 * acc) receives the old acc row and the row restarts from this state alone; every unmarked env's
 * ep_stats row is written all 0.  A row with n = 0 also starts from this state alone, without a
 * flush.  Otherwise the state is folded in: min for slots 1-4, +1 for n and for each count that
 * applies.
 *
 * The contract: call it once per state the policy acts on -- after hwy_reset (no mask), after
 * every step with that step's terminated / truncated, after a cut with its `cut`.  Under autoreset
 * the post-step state of a finished env is already the next episode's first state, so an episode's
 * measured states are s_0 .. s_{L-1}: its terminal state is not measured (the step's crashed flag,
 * hwy_step_with_info's episode sums, say how it ended).
 *
 * All pointers are device pointers and nullable, but at least one output (front, rear, gap,
 * closing, ttc, thw, risk, ego, acc) must be given.  hwy_traffic is asynchronous, allocates
 * nothing, is hipGraph-capturable, reads the state and writes nothing but the outputs it was
 * given.  It returns HWY_EINVAL before any device call for a NULL handle or NULL args, no output
 * at all, ep_stats or a restart mask without acc, and a ttc_thresh, thw_thresh, risk_horizon or
 * near_range that is not finite and positive.  On non-finite state words the neighbours are
 * whatever the step's neighbour rule gives for them and the values are not specified; the kernel
 * terminates and stays inside its outputs. */
#define HWY_TRAFFIC_NEGO 16
#define HWY_TRAFFIC_NACC 8
typedef struct hwy_traffic_args {
  int32_t* front;             /* device [E][64], nullable */
  int32_t* rear;              /* device [E][64], nullable */
  float* gap;                 /* device [E][64], nullable */
  float* closing;             /* device [E][64], nullable */
  float* ttc;                 /* device [E][64], nullable */
  float* thw;                 /* device [E][64], nullable */
  float* risk;                /* device [E][64], nullable */
  float* ego;                 /* device [E][HWY_TRAFFIC_NEGO], nullable */
  float* acc;                 /* device [E][HWY_TRAFFIC_NACC], in/out, nullable */
  float* ep_stats;            /* device [E][HWY_TRAFFIC_NACC], nullable; needs acc */
  const uint8_t* restart[3];  /* device [E] each, nullable; need acc */
  float ttc_thresh;           /* s, finite and > 0 */
  float thw_thresh;           /* s, finite and > 0 */
  float risk_horizon;         /* s, finite and > 0 */
  float near_range;           /* m, finite and > 0 */
} hwy_traffic_args;
/* sizeof(hwy_traffic_args) as compiled into the library (binding layout check). */
int hwy_traffic_args_size(void);
/* HWY_OK, or HWY_EINVAL for arguments hwy_traffic refuses (every check that needs no handle);
 * pure, no device call. */
int hwy_traffic_check(const hwy_traffic_args* a);
int hwy_traffic(hwy_handle* h, const hwy_traffic_args* a, void* stream);

/* ---- A sensor model in front of the observation: range, line of sight, missed detections and
 * measurement noise.
 *
 * hwy_sense observes all E envs from the state words as they stand, as hwy_observe does and
 * with the same observation code, but of the vehicles as a sensor on the ego perceives them: a
 * vehicle that is not `visible` is handed to the observation as absent, a visible one with a
 * perturbed x, y and speed.  Ranking, the 200 m perception test, see_behind, the shuffle and the
 * fused wrapper therefore act on the perceived vehicles, as they would on a tracker's list.  With
 * the null sensor (los 0, range_m +inf, p_drop 0, sigma 0 0 0) obs and row_vehicle are bit for
 * bit hwy_observe's.
 *
 * All arithmetic is binary32 without contraction, each product rounded before the sum it
 * enters; a comparison with a NaN is false.  The ego is vehicle 0 at (xe, ye), V =
 * vehicles_count + 1.  For vehicle k, 1 <= k < V, carrying HWY_FLAG_PRESENT:
 *   in range: dx = x_k - xe, dy = y_k - ye; in range iff dx*dx + dy*dy <= range_m*range_m
 *     (range_m = +inf: always).
 *   blocked (los != 0 only): some present j, 1 <= j < V, j != k, has its 5.0 x 2.0 rectangle at
 *     heading h_j meeting the segment from the ego's centre to k's centre.  A blocker is a body:
 *     it blocks whether or not it is visible itself.  In j's frame, by separating axes:
 *       (sj, cj) = hm_sincosf(h_j)
 *       ax = xe - x_j, ay = ye - y_j, bx = x_k - x_j, by = y_k - y_j
 *       u0 = ax*cj + ay*sj   w0 = ay*cj - ax*sj
 *       u1 = bx*cj + by*sj   w1 = by*cj - bx*sj
 *       blocked by j iff  min(u0,u1) <= 2.5 && max(u0,u1) >= -2.5
 *                      && min(w0,w1) <= 1.0 && max(w0,w1) >= -1.0
 *                      && |u0*w1 - u1*w0| <= 2.5*|w1 - w0| + 1.0*|u1 - u0|
 *   dropped: hm_u01(philox(k, step, 3, SALT, seed_lo, seed_hi).v[0]) < p_drop, with the env's
 *     step and seed words, philox = hm_philox4x32_10 (counter words, then key words) and
 *     SALT = 0x53454E53 + salt in uint32 (the shuffle's stream is 0x53485546).
 *   visible[k] = present && in range && !blocked && !dropped.  visible[0] is the ego's present
 *     bit; absent slots and k >= V give 0.
 *   noise, for channel c in {0: x, 1: y, 2: speed}: w = philox(k, step, c, SALT, seed_lo, seed_hi),
 *     u_i = hm_u01(w.v[i]), z_c = (((u_0 + u_1) + (u_2 + u_3)) - 2.0f) * 1.7320508f (zero mean,
 *     unit variance, |z| <= 2 sqrt 3); x' = x + sigma[0]*z_0, y' = y + sigma[1]*z_1,
 *     spd' = spd + sigma[2]*z_2.  A sigma of exactly 0 skips its addition (the bits of -0.0
 *     survive).  The heading and the ego are never perturbed.  Range and line of sight are
 *     decided on the true positions; the perceived ones enter the observation.
 *
 *   obs [E][N][F_out], row_vehicle [E][N] i32: as hwy_observe's, of the perceived vehicles,
 *     under `order` (-1: the handle's own).
 *   visible [E][64] u8: 1 / 0 as above.
 *   hidden [E][64] f32: 1.0 where present and not visible, else +0.0 (the ego: +0.0); hwy_render's
 *     `shade` layout.
 *   counts [E][4] i32: present others (1 <= k < V); of them out of range; in range but blocked;
 *     in range, not blocked but dropped.  The three and the visible others add up to the first.
 *
 * All output pointers are device pointers and nullable, but at least one must be given.
 * hwy_sense is asynchronous, allocates nothing, is hipGraph-capturable, reads the state and
 * writes nothing but the outputs it was given.  It returns HWY_EINVAL before any device call for
 * a NULL handle or NULL args, an order outside {-1, HWY_ORDER_SORTED, HWY_ORDER_SHUFFLED}, a
 * range_m that is neither +inf nor finite and > 0, a p_drop outside [0, 1], a sigma that is not
 * finite and >= 0, a salt outside 0..65535, no output at all, and a handle whose per-group PE
 * tables are without meaning (hwy_set_seed_groups).  On non-finite state words the values are
 * not specified; the kernel terminates and stays inside its outputs. */
#define HWY_SENSE_SALT 0x53454E53u
typedef struct hwy_sense_args {
  int32_t order;         /* -1: the handle's own; else enum hwy_order */
  int32_t los;           /* != 0: line-of-sight occlusion */
  float range_m;         /* m, finite and > 0, or +inf */
  float p_drop;          /* in [0, 1] */
  float sigma[3];        /* x (m), y (m), speed (m/s): finite and >= 0 */
  int32_t salt;          /* 0..65535 */
  float* obs;            /* device [E][N][F_out], nullable */
  int32_t* row_vehicle;  /* device [E][N], nullable */
  uint8_t* visible;      /* device [E][64], nullable */
  float* hidden;         /* device [E][64], nullable */
  int32_t* counts;       /* device [E][4], nullable */
} hwy_sense_args;
/* sizeof(hwy_sense_args) as compiled into the library (binding layout check). */
int hwy_sense_args_size(void);
/* HWY_OK, or HWY_EINVAL for arguments hwy_sense refuses (every check that needs no handle);
 * pure, no device call. */
int hwy_sense_check(const hwy_sense_args* a);
int hwy_sense(hwy_handle* h, const hwy_sense_args* a, void* stream);

/* ---- What-if rollouts of the stored states, and an action shield.
 *
 * hwy_lookahead runs K branches per env.  Branch (e, k) starts from env e's state words as they
 * stand and runs exactly what hwy_step runs on a handle with autoreset 0, up to `horizon` times:
 * the ego action of step h is mapped as ContinuousAction.act is (the step's own clip applies),
 * sim_freq / policy_freq frames follow, the step word goes up by 1, reward and terminated are the
 * step's expressions and truncated = step >= max_steps.  The branch ends after the first step with
 * terminated | truncated, or after `horizon` steps.  Nothing is ever reset, whatever the handle's
 * autoreset, and the handle's state is not written.  The frames draw no random numbers (Philox
 * enters only at reset and in the shuffled row order), so a branch is the future itself, bit for
 * bit: what `horizon` hwy_step calls on an autoreset-off handle holding a copy of the state
 * (hwy_export_state / hwy_import_state) return.
 *
 *   actions: hold != 0: [E][K][2], each held for all steps; else [E][K][H][2].
 *   steps [E][K] i32: the policy steps run, 1..H (0: not run, see lazy).
 *   terminated, truncated [E][K] u8: of the last step run.
 *   rewards [E][K][H] f32: the step's reward; +0.0 past `steps`.
 *   ret [E][K] f32, all in binary32: ret = 0, g = 1; per step run ret = ret + g * r, then
 *     g = g * gamma, each product rounded before the sum.  With gamma 1 this is the step's own
 *     running return.
 *   ego_final [E][K][4] f32: the ego's x, y, heading, speed after the last step run.
 *   obs [E][K][N][F_out] f32: what that autoreset-off hwy_step would have written on the
 *     branch's last step: under the branch's step count and the env's seed words (the shuffled
 *     order needs both), with the fused wrapper, and under hwy_set_seed_groups with the RankPE
 *     table of env e's group (indexed by the env, not by the branch).
 *   lazy != 0: candidates k >= 1 of an env run only if its candidate 0 terminated (two launches
 *     inside the call: k = 0, then k >= 1 reading terminated[e][0] behind it on the stream).  A
 *     branch that is skipped is written steps 0, flags 0 and +0.0 everywhere else.
 *   chosen [E] i32, chosen_action [E][2] f32 (one further small launch, integer logic only):
 *     candidate k is safe iff terminated[e][k] == 0 (a truncation or a full horizon is safe).
 *     chosen[e] is the least safe k; if none is safe, the k with the greatest steps[e][k], the
 *     least such k on ties.  Under lazy a safe candidate 0 is chosen without looking further.
 *     chosen_action[e] is the chosen candidate's first-step action, bits copied.
 *
 * No entry of a given output is left unwritten.  All outputs are device pointers and nullable,
 * but at least one must be given.  hwy_lookahead is asynchronous, allocates nothing, is
 * hipGraph-capturable and writes nothing but its outputs.  It returns HWY_EINVAL before any
 * device call for a NULL handle or NULL args, k or horizon outside 1..64, E * K above 2^22, a
 * gamma that is not finite or lies outside [0, 1], NULL actions, no output at all, lazy or chosen
 * without steps and terminated, chosen_action without chosen, and obs on a handle whose per-group
 * PE tables are without meaning (hwy_set_seed_groups).  On non-finite state words the values are
 * not specified; the kernel terminates and stays inside its outputs. */
#define HWY_LOOKAHEAD_MAX_K 64
#define HWY_LOOKAHEAD_MAX_H 64
#define HWY_LOOKAHEAD_MAX_BRANCHES (1 << 22)
typedef struct hwy_lookahead_args {
  int32_t k, horizon;     /* K candidates per env 1..64; H policy steps 1..64; E*K <= 2^22 */
  int32_t hold;           /* != 0: actions is [E][K][2], each held for all H steps; else [E][K][H][2] */
  int32_t lazy;           /* != 0: candidates k >= 1 of an env run only if its candidate 0 terminated */
  float gamma;            /* finite, 0 <= gamma <= 1 */
  const float* actions;   /* device, as `hold` says; the step's own clip applies */
  int32_t* steps;         /* [E][K]    policy steps run, 1..H (0: not run) */
  uint8_t* terminated;    /* [E][K]    of the last step run */
  uint8_t* truncated;     /* [E][K]    of the last step run */
  float* rewards;         /* [E][K][H] the step's reward; +0.0 past `steps` */
  float* ret;             /* [E][K]    see above */
  float* ego_final;       /* [E][K][4] the ego's x, y, heading, speed after the last step run */
  float* obs;             /* [E][K][N][F_out] the observation after the last step run */
  int32_t* chosen;        /* [E]       the shield's choice */
  float* chosen_action;   /* [E][2] */
} hwy_lookahead_args;
/* sizeof(hwy_lookahead_args) as compiled into the library (binding layout check). */
int hwy_lookahead_args_size(void);
/* HWY_OK, or HWY_EINVAL for arguments hwy_lookahead refuses (every check that needs no handle);
 * pure, no device call. */
int hwy_lookahead_check(const hwy_lookahead_args* a);
int hwy_lookahead(hwy_handle* h, const hwy_lookahead_args* a, void* stream);

/* ---- An occupancy grid of the env states: an observation without a row order.
 *
 * hwy_grid writes, for all E envs and from the state words as they stand, an ego-centred grid:
 * each vehicle goes into the cell its position falls in, so the result does not depend on any
 * ordering of the vehicles.  highway-env's OccupancyGridObservation is the model for the defaults
 * (the Python layer's), for the layout [C][W][H] (layer, cell along x, cell along y), for "the
 * lower vehicle index wins a cell" and for "empty cells are 0"; the rule itself is this project's
 * own, stated here, and is not pinned against upstream.  The grid observes a Kinematics env, as
 * hwy_sense does; "type": "OccupancyGrid" in an env config stays refused.
 *
 * All arithmetic is binary32 without contraction, each product rounded before the sum it
 * enters; a comparison with a NaN is false.  The ego is vehicle 0 at (xe, ye) with heading h_ego,
 * V = vehicles_count + 1, F the handle's n_features.
 *
 * Cell of vehicle k, 0 <= k < V, carrying HWY_FLAG_PRESENT (a flag word in a lane >= V means
 * nothing, as in the step):
 *   dx = x_k - xe, dy = y_k - ye
 *   align != 0: (s, c) = hm_sincosf(h_ego), u = dx*c + dy*s, w = dy*c - dx*s; else u = dx, w = dy
 *   qx = (u - x0) / step_x, qy = (w - y0) / step_y
 *   inside iff qx >= 0 && qx < nx && qy >= 0 && qy < ny, tested in float before any conversion:
 *     -0.0 is inside cell 0, an edge shared by two cells belongs to the upper one,
 *     x0 + nx*step_x is outside, and a non-finite position is outside and never becomes an index
 *   i = (int)floorf(qx), j = (int)floorf(qy), the flat cell is i*ny + j
 * Winner: the present, inside vehicle of least index wins its cell.  The ego is vehicle 0, so it
 * wins its own cell whenever it is inside the grid.  A crashed vehicle is drawn like any other.
 *
 *   grid [E][row_stride] f32: per env, n_layers layers of [nx][ny], then the ego tail, then
 *     padding.
 *     Vehicle layer l (layer_ids[l] an enum hwy_feature) in a won cell: the winner's feature value
 *       (the Kinematics observation's: vx = speed * cos h, ... with hm_sincosf of its heading); for
 *       x, y, vx and vy minus the ego's value of the same feature (the expression of the
 *       observation's relative rows, applied to the ego too, whose entries are therefore +0.0);
 *       then, where has_range[l], hm_lmap(., range[l][0], range[l][1], -1, 1) and, where clip,
 *       hm_clipf(., -1, 1).  Every other cell of the layer is +0.0.
 *     HWY_GRID_ON_ROAD layer: 1.0 where the cell's centre is on the road surface by hwy_render's
 *       layer-2 rule, else +0.0; vehicles do not touch it.  The centre is
 *       (gx, gy) = (x0 + ((float)i + 0.5f)*step_x, y0 + ((float)j + 0.5f)*step_y) in the grid's
 *       frame; under align (rx, ry) = (gx*c - gy*s, gx*s + gy*c), else (gx, gy); X = xe + rx,
 *       Y = ye + ry; on the road iff 0 <= X <= 10000 and -2 <= Y < 4*lanes_count - 2.
 *     Ego tail (ego_tail != 0): the F values of the handle's own Kinematics row 0 before any
 *       wrapper -- the ego's absolute feature values with the handle's normalize, has_range,
 *       features_range and clip as the observation applies them; on a handle without a wrapper,
 *       bit for bit, hwy_observe's row 0.
 *     Entries from the width n_layers*nx*ny + (ego_tail ? F : 0) up to row_stride are +0.0.
 *   cell_vehicle [E][nx][ny] i32: the winner of each cell, -1 for none.
 *   veh_cell [E][64] i32: the flat cell of each vehicle whether it won or not; -1 when it is
 *     outside the grid, absent, or k >= V.
 *   counts [E][4] i32, of the other vehicles (1 <= k < V): present; inside; inside but lost their
 *     cell; outside.  The second and the fourth add up to the first.
 *
 * No entry of a given output is left unwritten and nothing past E*row_stride floats of grid is
 * touched.  All outputs are device pointers and nullable, but at least one must be given.
 * hwy_grid is asynchronous, allocates nothing, is hipGraph-capturable, reads the state and writes
 * nothing but the outputs it was given.  It returns HWY_EINVAL before any device call for a NULL
 * handle or NULL args, no output at all, nx or ny below 1 or nx*ny above 1024, an x0 or y0 that
 * is not finite, a step that is not finite and > 0, n_layers outside 1..8, a layer id outside
 * 0..8 or given twice, a range (of a layer with has_range) with lo == hi or a bound that is not
 * finite, and a row_stride below the width or above 4096. */
#define HWY_GRID_ON_ROAD 8
#define HWY_GRID_MAX_LAYERS 8
#define HWY_GRID_MAX_CELLS 1024
#define HWY_GRID_MAX_STRIDE 4096
typedef struct hwy_grid_args {
  int32_t nx, ny;          /* cells along x and y, each >= 1, nx*ny <= 1024 */
  float x0, y0;            /* m, finite: the lower edge of cell 0, relative to the ego */
  float step_x, step_y;    /* m, finite and > 0 */
  int32_t align;           /* != 0: the ego's axes instead of the road's */
  int32_t n_layers;        /* 1..8 */
  int32_t layer_ids[HWY_GRID_MAX_LAYERS];  /* enum hwy_feature or HWY_GRID_ON_ROAD, distinct */
  int32_t has_range[HWY_GRID_MAX_LAYERS];  /* layer has a range */
  float range[HWY_GRID_MAX_LAYERS][2];     /* [lo, hi] per layer, finite, lo != hi */
  int32_t clip;            /* != 0: clip ranged layers to [-1, 1] */
  int32_t ego_tail;        /* != 0: append the ego's own Kinematics row */
  int32_t row_stride;      /* floats per env in grid: width..4096 */
  float* grid;             /* device [E][row_stride], nullable */
  int32_t* cell_vehicle;   /* device [E][nx][ny], nullable */
  int32_t* veh_cell;       /* device [E][64], nullable */
  int32_t* counts;         /* device [E][4], nullable */
} hwy_grid_args;
/* sizeof(hwy_grid_args) as compiled into the library (binding layout check). */
int hwy_grid_args_size(void);
/* HWY_OK, or HWY_EINVAL for arguments hwy_grid refuses (every check that needs no handle: of
 * row_stride, that it holds the layers, one more float with ego_tail, and is at most 4096; the
 * handle's F enters in hwy_grid); pure, no device call. */
int hwy_grid_check(const hwy_grid_args* a);
int hwy_grid(hwy_handle* h, const hwy_grid_args* a, void* stream);

/* ---- A ray-cast range observation of the env states: a ring of lidar returns around the ego.
 *
 * hwy_lidar casts, for all E envs and from the state words as they stand, n = cells*sub rays from
 * the ego's centre against the 5.0 x 2.0 rectangles of the other present vehicles and writes per
 * cell the nearest return: (distance, relative radial speed).  Like the grid it has no row order;
 * unlike it, it is narrow (2*cells floats) and occlusion-aware by construction: a car behind
 * another returns nothing.  highway-env's LidarObservation is the model for the shape: the layout
 * [cells][2], cell i centred on direction i*2pi/cells, and the config keys cells, maximum_range
 * and normalize (the Python layer takes them over).  The rule itself is this project's own, stated
 * here, and is not pinned against upstream's trace(): upstream's "centre distance minus half a
 * width" shortcut for the sector that holds a vehicle's centre is not reproduced; instead a cell
 * may pool several sub-rays.  Road borders are no returns.  The lidar observes a Kinematics env;
 * "type": "LidarObservation" in an env config stays refused.
 *
 * All arithmetic is binary32 without contraction, each product rounded before the sum it
 * enters; a comparison with a NaN is false; min(a, b) is b < a ? b : a and max(a, b) is
 * b > a ? b : a.  The ego is vehicle 0 at (xe, ye) with heading h_e, V = vehicles_count + 1, F
 * the handle's n_features.  A vehicle k, 1 <= k < V, is a body iff it carries HWY_FLAG_PRESENT (a
 * flag word in a lane >= V means nothing, as in the step).  A crashed vehicle is a body.
 *
 * Rays.  dth = (float)(6.283185307179586 / (double)n), computed in the library.  Sub-ray j of cell
 * i, r = i*sub + j:
 *   theta = ((float)r + (0.5f - 0.5f*(float)sub)) * dth; with align != 0, theta = theta + h_e
 *   (dy, dx) = hm_sincosf(theta)
 * so sub = 1 gives upstream's directions and a cell's sub-rays are spread evenly about its centre.
 *
 * Ray against body k, the slab test in the body's frame:
 *   (sk, ck) = hm_sincosf(h_k), ox = xe - x_k, oy = ye - y_k
 *   ou = ox*ck + oy*sk, ow = oy*ck - ox*sk, du = dx*ck + dy*sk, dw = dy*ck - dx*sk
 *   per axis a with half extent H (2.5 for u, 1.0 for w):
 *     d_a == 0: the interval is (-inf, +inf) when |o_a| <= H, else empty
 *     otherwise t1 = (-H - o_a)/d_a, t2 = (H - o_a)/d_a, the interval is [min(t1,t2), max(t1,t2)]
 *   t_in = max(lower end of u, lower end of w), t_out = min(upper end of u, upper end of w)
 *   the ray hits k iff neither interval is empty, t_in <= t_out and t_out >= 0
 *   its distance is d = t_in > 0 ? t_in : +0.0: an origin inside the rectangle gives 0
 *   the hit counts iff d <= range_m
 * The d_a == 0 branch is no corner case: the unaligned ray 0 against a heading-0 body has dw == 0
 * exactly.  A body whose position or heading is not finite returns nothing: every t of it is then
 * non-finite and fails one of the tests above.
 *
 * Winners.  A ray returns its counted hit of least d, among equal d the least k.  A cell returns
 * its sub-ray of least d, among equal d the least j.  A returning cell has
 *   dist = d, vel = ((vkx - vex)*dx) + ((vky - vey)*dy)
 * with dx, dy of the winning sub-ray and v?x = speed*cos, v?y = speed*sin from hm_sincosf of the
 * stored headings.  A cell without a return has dist = range_m, vel = +0.0, hit_vehicle = -1.
 *
 * Per-cell sensor errors, after pooling, keyed like hwy_sense's draws:
 *   w(c) = philox4x32_10((cell, step word, c, HWY_LIDAR_SALT + salt), key = the episode's seed)
 *   c = 0, dropout: the cell is dropped iff hm_u01(w(0)[0]) < p_drop, whether it returned or not;
 *     a dropped cell is written as a cell without a return
 *   c = 1, range noise, on cells that return and are not dropped: with hwy_sense's
 *     z = (((u0 + u1) + (u2 + u3)) - 2) * 1.7320508f of w(1),
 *     dist = hm_clipf(dist + sigma_r*z, 0, range_m); a sigma_r of exactly 0 skips the addition.
 *   The range test is on the true distance, before the noise.
 *
 *   obs [E][row_stride] f32: per env the cells pairs (dist, vel), with normalize != 0 as
 *     (dist / range_m, vel / speed_scale); then, with ego_tail != 0, the F values of the handle's
 *     own Kinematics row 0 before any wrapper (exactly hwy_grid's ego tail); entries from the
 *     width 2*cells + (ego_tail ? F : 0) up to row_stride are +0.0.
 *   hit_vehicle [E][cells] i32: the vehicle a cell returns, -1 for none.
 *   seen [E][64] f32: 1.0 where the vehicle is the return of at least one undropped cell, else
 *     +0.0 (the ego, absent slots and lanes >= V included): hwy_render's shade layout.
 *   counts [E][4] i32: bodies (present others); bodies seen; cells with a return; cells dropped.
 *
 * No entry of a given output is left unwritten and nothing past E*row_stride floats of obs is
 * touched.  All outputs are device pointers and nullable, but at least one must be given.
 * hwy_lidar is asynchronous, allocates nothing, is hipGraph-capturable, reads the state and
 * writes nothing but the outputs it was given.  On non-finite state words the values are
 * unspecified, but every loop is bounded and every index in bounds.  It returns HWY_EINVAL before
 * any device call for a NULL handle or NULL args, no output at all, cells outside 1..1024, sub
 * outside 1..16, cells*sub above 4096, a range_m or speed_scale that is not finite and > 0, a
 * p_drop outside [0, 1], a sigma_r that is not finite and >= 0, a salt outside 0..65535 and a
 * row_stride below the width or above 4096. */
#define HWY_LIDAR_SALT 0x4C494441u
#define HWY_LIDAR_MAX_CELLS 1024
#define HWY_LIDAR_MAX_SUB 16
#define HWY_LIDAR_MAX_RAYS 4096
#define HWY_LIDAR_MAX_STRIDE 4096
typedef struct hwy_lidar_args {
  int32_t cells;         /* 1..1024 */
  int32_t sub;           /* sub-rays per cell, 1..16, cells*sub <= 4096 */
  float range_m;         /* m, finite and > 0 */
  int32_t align;         /* != 0: cell 0 points along the ego's heading, not the road's x */
  int32_t normalize;     /* != 0: dist / range_m, vel / speed_scale */
  float speed_scale;     /* m/s, finite and > 0 */
  float p_drop;          /* per-cell dropout probability, 0..1 */
  float sigma_r;         /* m, range noise, finite and >= 0 */
  int32_t salt;          /* 0..65535 */
  int32_t ego_tail;      /* != 0: append the ego's own Kinematics row */
  int32_t row_stride;    /* floats per env in obs: width..4096 */
  float* obs;            /* device [E][row_stride], nullable */
  int32_t* hit_vehicle;  /* device [E][cells], nullable */
  float* seen;           /* device [E][64], nullable */
  int32_t* counts;       /* device [E][4], nullable */
} hwy_lidar_args;
/* sizeof(hwy_lidar_args) as compiled into the library (binding layout check). */
int hwy_lidar_args_size(void);
/* HWY_OK, or HWY_EINVAL for arguments hwy_lidar refuses (every check that needs no handle: of
 * row_stride, that it holds the cells, one more float with ego_tail, and is at most 4096; the
 * handle's F enters in hwy_lidar); pure, no device call. */
int hwy_lidar_check(const hwy_lidar_args* a);
int hwy_lidar(hwy_handle* h, const hwy_lidar_args* a, void* stream);

/* Stand-alone observation wrapper on [E,N,F] f32 -> [E,N,F_out] f32 (foreign envs).
 *   kind = enum hwy_pe_kind, d = appended width (rank/dist) or rotate_dim (rope),
 *   table = device pointer as for hwy_set_pe_table. dist_override (nullable, [E,N]) replaces
 *   the computed normalised distance (RotaryEmbedWrapper._apply_rope(obs, dist_norm)). */
int hwy_obs_pe(const float* obs_in, float* obs_out, int E, int N, int F, int kind, int d,
               int ego_idx, float max_dist, const float* table, const float* dist_override,
               void* stream);

/* GAE over a [T,E] rollout (ppo/agent.py:126-138): float64 arithmetic, float32 storage,
 * done = terminated|truncated treated as terminal (training/routine.py:135). */
int hwy_gae(const float* rewards, const uint8_t* dones, const float* values,
            const float* last_values, double gamma, double lam, int T, int E, float* advantages,
            float* returns, void* stream);

/* hwy_gae with a bootstrap at truncation; every array [T,E].  Per step, with v1 the next step's
 * value (last_values past the end) and last_adv the next step's advantage:
 *   done = term | trunc;  boot = trunc & !term;  vsel = boot ? boot_values[i] : v1
 *   m = (done && !boot) ? 0 : 1;  nd = done ? 0 : 1
 *   delta = (r + (gamma * vsel) * m) - v0;  a = (float)(delta + (gamma*lam * nd) * last_adv)
 * in float64, each step rounded to float32, ret = a + v0: a truncated row's advantage is its
 * one-step TD error against V(final observation) and the chain is cut there.  Without a boot row
 * the result is hwy_gae's on dones = term | trunc, bit for bit. */
int hwy_gae_boot(const float* rewards, const uint8_t* terminated, const uint8_t* truncated,
                 const float* values, const float* last_values, const float* boot_values,
                 double gamma, double lam, int T, int E, float* advantages, float* returns,
                 void* stream);

/* Device self-test of the deterministic math library (tests only): out[i] = op(in[i], in2[i]). */
int hwy_math_selftest(int op, const float* in, const float* in2, float* out, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HWY_H_ */
