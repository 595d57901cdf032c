// hwy_internal.h -- launch parameters shared by hwy_api.cpp (host) and hwy_kernels.hip.
#ifndef HWY_INTERNAL_H_
#define HWY_INTERNAL_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hwy.h"

struct StepParams {
  hwy_config cfg;
  uint32_t* state;
  const float* actions;
  float* obs;
  float* reward;
  uint8_t* term;
  uint8_t* trunc;
  float* ep_ret;
  int32_t* ep_len;
  const float* pe_table;
  const uint64_t* seeds;
  const uint8_t* mask;
  int fout;
  // experiment groups (hwy_set_seed_groups): per-group seed bases, envs per group, and the
  // floats between consecutive groups' PE tables (0: one table for all)
  const int64_t* group_seed;
  int group_envs;
  int pe_group_stride;
};

// the info kernels' second argument (solo) / second table's record (grouped): the ABI's struct
typedef hwy_step_info InfoParams;

// the final kernels' second argument / second table's record: the info pointers (all NULL when
// the caller wants none) and the terminal observations' buffer [E, N, F_out]
struct FinalParams {
  InfoParams info;
  float* final_obs;
};

// hwy_render's launch parameters (hwy_render.hip): the checked arguments and the handle's state
struct RenderParams {
  hwy_render_args a;
  const uint32_t* state;  // [HWY_NFIELDS][E][64]
  int num_envs, lanes_count;
};

// hwy_observe's launch parameters (the observe unit of hwy_kernels.hip): p.cfg is the handle's
// config with the order the call asked for, p.obs the (nullable) observation output; the rest of
// the outputs as in hwy_observe_args
struct ObserveParams {
  StepParams p;
  int32_t* row_vehicle;
  const float* row_values;
  float* veh_values;
};

// hwy_traffic's launch parameters (the traffic unit of hwy_kernels.hip): the checked arguments,
// the handle's state and its config (the neighbour search takes the config it takes in the step)
struct TrafficParams {
  hwy_traffic_args a;
  const uint32_t* state;  // [HWY_NFIELDS][E][64]
  hwy_config cfg;
};

// hwy_sense's launch parameters (the sense unit of hwy_kernels.hip): p as in ObserveParams
// (p.obs = a.obs), a the checked arguments, salt_word = HWY_SENSE_SALT + a.salt, range2 =
// a.range_m * a.range_m (+inf for +inf)
struct SenseParams {
  StepParams p;
  hwy_sense_args a;
  uint32_t salt_word;
  float range2;
  float cull2;  // ((a.range_m + 4) * 1.0001)^2: a body farther from the ego blocks nothing in range
};

// hwy_lookahead's launch parameters (the lookahead unit of hwy_kernels.hip): p the handle's own
// (its state is only read), a the checked arguments; the launch runs candidates k0 .. k0 + nk - 1
// of every env, and with gate != 0 only those of envs whose terminated[e][0] is set
struct LookaheadParams {
  StepParams p;
  hwy_lookahead_args a;
  int k0, nk, gate;
};

// hwy_grid's launch parameters (the grid unit of hwy_kernels.hip): the checked arguments, the
// handle's state and its config (V, lanes_count and the ego tail's features and ranges)
struct GridParams {
  hwy_grid_args a;
  const uint32_t* state;  // [HWY_NFIELDS][E][64]
  hwy_config cfg;
};

// hwy_lidar's launch parameters (the lidar unit of hwy_kernels.hip): the checked arguments, the
// handle's state and its config, dth = (float)(2 pi / (cells * sub)), salt_word =
// HWY_LIDAR_SALT + a.salt and cull2 = ((range_m + 4) * 1.0001)^2, the squared centre distance
// beyond which no ray can count a hit on a body
struct LidarParams {
  hwy_lidar_args a;
  const uint32_t* state;  // [HWY_NFIELDS][E][64]
  hwy_config cfg;
  float dth;
  uint32_t salt_word;
  float cull2;
};

extern "C" {
int hwy_launch_grid(const GridParams* p, hipStream_t s);
int hwy_launch_lidar(const LidarParams* p, hipStream_t s);
// big: the register budget, hwy_step_big(waves of the launch)
int hwy_launch_lookahead(const LookaheadParams* p, int big, hipStream_t s);
int hwy_launch_lookahead_choice(const LookaheadParams* p, hipStream_t s);
int hwy_launch_sense(const SenseParams* p, hipStream_t s);
int hwy_launch_traffic(const TrafficParams* p, hipStream_t s);
int hwy_launch_observe(const ObserveParams* p, hipStream_t s);
int hwy_launch_render(const RenderParams* p, hipStream_t s);
int hwy_launch_step(const StepParams* p, hipStream_t s);
// n handles' steps in one launch: dtab = n StepParams in device memory, blocks = the largest
// handle's hwy_step_blocks, big = hwy_step_big(total envs) (the register budget of the launch)
int hwy_launch_step_group(const StepParams* dtab, int n, int blocks, int big, hipStream_t s);
// the info variants (their own unit): info / itab as above, the rest as the plain launches
int hwy_launch_step_info(const StepParams* p, const InfoParams* info, hipStream_t s);
int hwy_launch_step_group_info(const StepParams* dtab, const InfoParams* itab, int n, int blocks,
                               int big, hipStream_t s);
// the final variants (their own unit): the info variants plus the terminal observation
int hwy_launch_step_final(const StepParams* p, const FinalParams* f, hipStream_t s);
int hwy_launch_step_group_final(const StepParams* dtab, const FinalParams* ftab, int n, int blocks,
                                int big, hipStream_t s);
int hwy_step_blocks(int num_envs);
int hwy_step_big(int64_t total_envs);
int hwy_launch_reset(const StepParams* p, hipStream_t s);
// hwy_cut_episodes: p->obs / ep_ret / ep_len as for a step, cut [E] u8 (nullable)
int hwy_launch_cut(const StepParams* p, uint8_t* cut, hipStream_t s);
int hwy_launch_obs_pe(const float* in, float* out, int E, int N, int F, int kind, int d, int ego,
                      float max_dist, const float* table, const float* dov, hipStream_t s);
int hwy_launch_gae(const float* rew, const uint8_t* done, const float* val, const float* last_val,
                   double gamma, double lam, int T, int E, float* adv, float* ret, hipStream_t s);
int hwy_launch_gae_boot(const float* rew, const uint8_t* term, const uint8_t* trunc,
                        const float* val, const float* last_val, const float* bootv, double gamma,
                        double lam, int T, int E, float* adv, float* ret, hipStream_t s);
int hwy_launch_math(int op, const float* in, const float* in2, float* out, int n, hipStream_t s);
}
#endif
