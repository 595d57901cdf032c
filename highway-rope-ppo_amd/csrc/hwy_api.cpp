// hwy_api.cpp -- the C ABI of libhwy.so (include/hwy.h): handle management, validation and
// launches.  No allocation, copy or synchronisation happens inside the compute entry points
// (hwy_reset / hwy_step / hwy_obs_pe / hwy_gae), so callers may capture them in a hipGraph.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hwy.h"
#include "hwy_internal.h"

struct hwy_handle {
  hwy_config cfg;
  int device;
  int fout;
  uint32_t* state;  // [HWY_NFIELDS][E][64]
  float* pe_table;  // [HWY_MAX_PE_TABLE]
  int64_t* group_seed;  // [n_groups] (hwy_set_seed_groups), or null
  int n_groups, group_envs, pe_group_stride;
  // the per-group RankPE tables no longer match the groups (hwy_set_seed_groups changed their
  // geometry): every launch and prepare is refused until hwy_set_pe_table loads a table again
  int pe_invalid;
};

static thread_local char g_err[512];

static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

static int hip_fail(hipError_t e, const char* what) {
  return fail(HWY_EDEVICE, "%s: %s", what, hipGetErrorString(e));
}

// the end of every compute entry point: rc is a hwy_launch_*'s return
static int launched(int rc, const char* kernel) {
  return rc ? hip_fail(hipGetLastError(), kernel) : HWY_OK;
}

static bool finite_pos(float x) { return x > 0.0f && x < __builtin_inff(); }

static int pe_extra(const hwy_config* c) {
  return (c->pe_kind == HWY_PE_RANK || c->pe_kind == HWY_PE_DIST || c->pe_kind == HWY_PE_DIST1)
             ? c->d_embed
             : 0;
}

static int validate(const hwy_config* c) {
  if (!c) return fail(HWY_EINVAL, "config is NULL");
  if (c->num_envs < 1) return fail(HWY_EINVAL, "num_envs must be >= 1, got %d", c->num_envs);
  if (c->num_envs > (1 << 26) - 1)  // state words of one field indexed with 32 bits on device
    return fail(HWY_EINVAL, "num_envs must be < 2^26 per handle, got %d", c->num_envs);
  if (c->lanes_count < 1 || c->lanes_count > 64)
    return fail(HWY_EINVAL, "lanes_count must be in [1, 64], got %d", c->lanes_count);
  if (c->vehicles_count < 0 || c->vehicles_count + 1 > HWY_MAX_VEHICLES)
    return fail(HWY_EINVAL, "vehicles_count must be in [0, %d], got %d", HWY_MAX_VEHICLES - 1,
                c->vehicles_count);
  if (c->obs_vehicles < 1 || c->obs_vehicles > HWY_MAX_OBS_ROWS)
    return fail(HWY_EINVAL, "observation vehicles_count must be in [1, %d], got %d",
                HWY_MAX_OBS_ROWS, c->obs_vehicles);
  if (c->n_features < 1 || c->n_features > HWY_MAX_FEATURES)
    return fail(HWY_EINVAL, "feature count must be in [1, %d], got %d", HWY_MAX_FEATURES,
                c->n_features);
  for (int f = 0; f < c->n_features; ++f)
    if (c->feature_ids[f] < 0 || c->feature_ids[f] > HWY_FEAT_HEADING)
      return fail(HWY_EINVAL, "unsupported feature id %d", c->feature_ids[f]);
  if (c->order != HWY_ORDER_SORTED && c->order != HWY_ORDER_SHUFFLED)
    return fail(HWY_EINVAL, "order must be sorted or shuffled");
  if (c->sim_freq < 1 || c->policy_freq < 1 || c->sim_freq < c->policy_freq)
    return fail(HWY_EINVAL, "simulation_frequency (%d) must be >= policy_frequency (%d) >= 1",
                c->sim_freq, c->policy_freq);
  if (c->max_steps < 1) return fail(HWY_EINVAL, "max_steps must be >= 1");
  if (c->initial_lane_id >= c->lanes_count)
    return fail(HWY_EINVAL, "initial_lane_id %d out of range", c->initial_lane_id);
  if (!(c->vehicles_density > 0.0f)) return fail(HWY_EINVAL, "vehicles_density must be > 0");
  switch (c->pe_kind) {
    case HWY_PE_NONE: break;
    case HWY_PE_RANK:
      if (c->d_embed < 1) return fail(HWY_EINVAL, "d_embed must be >= 1 for RankPE");
      break;
    case HWY_PE_DIST:
      if (c->d_embed < 2 || c->d_embed % 2)
        return fail(HWY_EINVAL, "DistanceEmbedWrapper requires even d_embed; got %d", c->d_embed);
      if (c->n_features < 2) return fail(HWY_EINVAL, "DistPE needs at least 2 features");
      break;
    case HWY_PE_DIST1:
      if (c->d_embed < 2 || c->d_embed % 2)
        return fail(HWY_EINVAL, "DistanceEmbedWrapper requires even d_embed; got %d", c->d_embed);
      break;
    case HWY_PE_ROPE:
      if (c->d_embed % 2 || c->d_embed > c->n_features || c->d_embed < 0)
        return fail(HWY_EINVAL, "rotate_dim must be even and <= %d; got %d", c->n_features,
                    c->d_embed);
      if (c->n_features < 2) return fail(HWY_EINVAL, "RoPE needs at least 2 features");
      break;
    default: return fail(HWY_EINVAL, "unknown pe_kind %d", c->pe_kind);
  }
  if (c->n_features + pe_extra(c) > HWY_MAX_FOUT)
    return fail(HWY_EINVAL, "F + d_embed exceeds %d", HWY_MAX_FOUT);
  if (c->ego_idx < 0 || c->ego_idx >= c->obs_vehicles)
    return fail(HWY_EINVAL, "ego_idx %d out of range", c->ego_idx);
  if (!(c->pe_max_dist > 0.0f)) return fail(HWY_EINVAL, "max_dist must be > 0");
  return HWY_OK;
}

static size_t state_bytes(const hwy_handle* h) {
  return (size_t)HWY_NFIELDS * (size_t)h->cfg.num_envs * HWY_MAX_VEHICLES * sizeof(uint32_t);
}

extern "C" {

int hwy_abi_version(void) { return HWY_ABI_VERSION; }

int hwy_config_size(void) { return (int)sizeof(hwy_config); }

const char* hwy_last_error(void) { return g_err; }

int hwy_create(const hwy_config* cfg, int device, hwy_handle** out) {
  if (!out) return fail(HWY_EINVAL, "out is NULL");
  *out = nullptr;
  int rc = validate(cfg);
  if (rc) return rc;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  hwy_handle* h = new hwy_handle();
  h->cfg = *cfg;
  h->device = device;
  h->fout = cfg->n_features + pe_extra(cfg);
  const char* what = "hipMalloc(state)";
  e = hipMalloc(&h->state, state_bytes(h));
  if (e == hipSuccess) {
    what = "hipMalloc(pe_table)";
    e = hipMalloc(&h->pe_table, HWY_MAX_PE_TABLE * sizeof(float));
  }
  if (e == hipSuccess) {
    what = "hipMemset";
    (void)hipMemset(h->state, 0, state_bytes(h));
    (void)hipMemset(h->pe_table, 0, HWY_MAX_PE_TABLE * sizeof(float));
    e = hipDeviceSynchronize();
  }
  if (e != hipSuccess) {
    hwy_destroy(h);  // frees what exists of h
    return hip_fail(e, what);
  }
  *out = h;
  return HWY_OK;
}

// also hwy_create's error path: h may be partly built (hipFree(NULL) does nothing)
void hwy_destroy(hwy_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(h->state);
  (void)hipFree(h->pe_table);
  (void)hipFree(h->group_seed);
  delete h;
}

int hwy_obs_features(const hwy_handle* h) { return h ? h->fout : HWY_EINVAL; }

int hwy_set_pe_table(hwy_handle* h, const float* table_host, int n) {
  if (!h) return fail(HWY_EINVAL, "handle is NULL");
  const hwy_config& c = h->cfg;
  int need = 0;
  if (c.pe_kind == HWY_PE_RANK) need = c.obs_vehicles * c.d_embed;
  if (c.pe_kind == HWY_PE_DIST || c.pe_kind == HWY_PE_DIST1) need = c.d_embed / 2;
  if (c.pe_kind == HWY_PE_ROPE) need = c.d_embed / 2;
  int stride = 0;
  if (c.pe_kind == HWY_PE_RANK && h->n_groups > 0 && n == need * h->n_groups && n != need) {
    stride = need;  // one RankPE table per experiment group
    need = n;
  }
  if (n != need) return fail(HWY_EINVAL, "pe table needs %d floats, got %d", need, n);
  if (n > HWY_MAX_PE_TABLE) return fail(HWY_EINVAL, "pe table too large (%d)", n);
  if (n == 0) return HWY_OK;
  (void)hipSetDevice(h->device);
  hipError_t e = hipMemcpy(h->pe_table, table_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpy(pe_table)");
  h->pe_group_stride = stride;
  h->pe_invalid = 0;
  return HWY_OK;
}

int hwy_set_seed_groups(hwy_handle* h, const int64_t* seed_bases, int n_groups, int envs_per_group) {
  if (!h) return fail(HWY_EINVAL, "handle is NULL");
  (void)hipSetDevice(h->device);
  if (n_groups == 0) {
    if (h->group_seed) (void)hipFree(h->group_seed);
    h->group_seed = nullptr;
    if (h->pe_group_stride) h->pe_invalid = 1;  // per-group tables without groups
    h->n_groups = h->group_envs = h->pe_group_stride = 0;
    return HWY_OK;
  }
  if (!seed_bases || n_groups < 0 || envs_per_group < 1 ||
      (int64_t)n_groups * envs_per_group != h->cfg.num_envs)
    return fail(HWY_EINVAL, "seed groups: %d groups x %d envs must cover num_envs %d", n_groups,
                envs_per_group, h->cfg.num_envs);
  int64_t* dev = nullptr;
  hipError_t e = hipMalloc(&dev, (size_t)n_groups * sizeof(int64_t));
  if (e != hipSuccess) return hip_fail(e, "hipMalloc(group_seed)");
  e = hipMemcpy(dev, seed_bases, (size_t)n_groups * sizeof(int64_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(dev);
    return hip_fail(e, "hipMemcpy(group_seed)");
  }
  if (h->group_seed) (void)hipFree(h->group_seed);
  h->group_seed = dev;
  // per-group RankPE tables (hwy_set_pe_table after the groups) stay with groups of the same
  // geometry: group g keeps reading table g.  Any other geometry leaves them meaningless.
  if (h->pe_group_stride && (n_groups != h->n_groups || envs_per_group != h->group_envs)) {
    h->pe_group_stride = 0;
    h->pe_invalid = 1;
  }
  h->n_groups = n_groups;
  h->group_envs = envs_per_group;
  return HWY_OK;
}

int hwy_set_seed_schedule(hwy_handle* h, int64_t seed_base, int32_t env_offset, int64_t seed_stride) {
  if (!h) return fail(HWY_EINVAL, "handle is NULL");
  if (seed_stride < 0) return fail(HWY_EINVAL, "seed_stride must be >= 0");
  h->cfg.seed_base = seed_base;
  h->cfg.env_offset = env_offset;
  h->cfg.seed_stride = seed_stride;
  return HWY_OK;
}

static int check_pe(const hwy_handle* h, const char* who) {
  if (h->pe_invalid)
    return fail(HWY_EINVAL, "%s: the per-group PE tables were loaded for other seed groups; call "
                            "hwy_set_pe_table again", who);
  return HWY_OK;
}

static StepParams params_of(hwy_handle* h) {
  StepParams p;
  memset(&p, 0, sizeof(p));
  p.cfg = h->cfg;
  p.state = h->state;
  p.pe_table = h->pe_table;
  p.fout = h->fout;
  p.group_seed = h->group_seed;
  p.group_envs = h->group_envs;
  p.pe_group_stride = h->pe_group_stride;
  return p;
}

static bool step_io_ok(const hwy_step_io& a) {
  return a.actions && a.obs && a.reward && a.terminated && a.truncated;
}

static int check_step_io(const char* who, const hwy_step_io& a) {
  if (!step_io_ok(a))
    return fail(HWY_EINVAL, "%s: actions/obs/reward/terminated/truncated must be non-NULL", who);
  return HWY_OK;
}

// params_of(h) with one step's buffers
static StepParams step_params(hwy_handle* h, const hwy_step_io& a) {
  StepParams p = params_of(h);
  p.actions = a.actions;
  p.obs = a.obs;
  p.reward = a.reward;
  p.term = a.terminated;
  p.trunc = a.truncated;
  p.ep_ret = a.ep_return;
  p.ep_len = a.ep_length;
  return p;
}

// a grouped variant's second device table, after hwy_step_group_prepare filled the first
static int upload_table(void* dst, const void* src, size_t bytes, void* stream, const char* who) {
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return e == hipSuccess ? HWY_OK : hip_fail(e, who);
}

int hwy_reset(hwy_handle* h, const uint64_t* seeds, const uint8_t* mask, float* obs, void* stream) {
  if (!h) return fail(HWY_EINVAL, "handle is NULL");
  if (int rc = check_pe(h, "hwy_reset")) return rc;
  StepParams p = params_of(h);
  p.seeds = seeds;
  p.mask = mask;
  p.obs = obs;
  return launched(hwy_launch_reset(&p, (hipStream_t)stream), "hwy_reset_kernel");
}

int hwy_step(hwy_handle* h, const float* actions, float* obs, float* reward, uint8_t* terminated,
             uint8_t* truncated, float* ep_return, int32_t* ep_length, void* stream) {
  if (!h) return fail(HWY_EINVAL, "handle is NULL");
  const hwy_step_io io = {actions, obs, reward, terminated, truncated, ep_return, ep_length};
  if (int rc = check_step_io("hwy_step", io)) return rc;
  if (int rc = check_pe(h, "hwy_step")) return rc;
  const StepParams p = step_params(h, io);
  return launched(hwy_launch_step(&p, (hipStream_t)stream), "hwy_step_kernel");
}

int hwy_step_info_size(void) { return (int)sizeof(hwy_step_info); }

// the info variants' and (where info is given) the final variants' rule on the info pointers
static int check_ep_stats(const hwy_step_info* info, const char* who) {
  if (info && info->ep_stats && !info->acc)
    return fail(HWY_EINVAL, "%s: ep_stats needs acc (the episode's running sums)", who);
  return HWY_OK;
}

static int check_info(const hwy_step_info* info, const char* who) {
  if (!info) return fail(HWY_EINVAL, "%s: info is NULL", who);
  return check_ep_stats(info, who);
}

int hwy_step_with_info(hwy_handle* h, const float* actions, float* obs, float* reward,
                       uint8_t* terminated, uint8_t* truncated, float* ep_return,
                       int32_t* ep_length, const hwy_step_info* info, void* stream) {
  if (!h) return fail(HWY_EINVAL, "handle is NULL");
  const hwy_step_io io = {actions, obs, reward, terminated, truncated, ep_return, ep_length};
  if (int rc = check_step_io("hwy_step_with_info", io)) return rc;
  if (int rc = check_info(info, "hwy_step_with_info")) return rc;
  if (int rc = check_pe(h, "hwy_step_with_info")) return rc;
  const StepParams p = step_params(h, io);
  return launched(hwy_launch_step_info(&p, info, (hipStream_t)stream), "hwy_step_info_kernel");
}

int hwy_cut_episodes(hwy_handle* h, float* obs, float* ep_return, int32_t* ep_length,
                     uint8_t* cut, void* stream) {
  if (!h) return fail(HWY_EINVAL, "handle is NULL");
  if (!obs) return fail(HWY_EINVAL, "hwy_cut_episodes: obs must be non-NULL");
  if (int rc = check_pe(h, "hwy_cut_episodes")) return rc;
  StepParams p = params_of(h);
  p.obs = obs;
  p.ep_ret = ep_return;
  p.ep_len = ep_length;
  return launched(hwy_launch_cut(&p, cut, (hipStream_t)stream), "hwy_cut_kernel");
}

int64_t hwy_step_group_table_bytes(int n) {
  return n < 1 ? -1 : (int64_t)n * (int64_t)sizeof(StepParams);
}

int hwy_step_group_prepare(hwy_handle* const* handles, const hwy_step_io* io, int n, void* table,
                           hwy_step_group_plan* plan, void* stream) {
  if (!handles || !io || n < 1 || !table || !plan)
    return fail(HWY_EINVAL, "hwy_step_group_prepare: handles/io/table/plan NULL or n < 1");
  std::vector<StepParams> tab(n);
  int blocks = 0, dev = -1;
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    hwy_handle* h = handles[i];
    const hwy_step_io& a = io[i];
    if (!h || !step_io_ok(a))
      return fail(HWY_EINVAL, "hwy_step_group_prepare: handle %d or its actions/obs/reward/"
                              "terminated/truncated is NULL", i);
    if (dev >= 0 && h->device != dev)
      return fail(HWY_EINVAL, "hwy_step_group_prepare: handles on devices %d and %d", dev,
                  h->device);
    dev = h->device;
    if (int rc = check_pe(h, "hwy_step_group_prepare")) return rc;
    tab[i] = step_params(h, a);
    const int b = hwy_step_blocks(h->cfg.num_envs);
    blocks = b > blocks ? b : blocks;
    total += h->cfg.num_envs;
  }
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipStreamSynchronize(s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(table, tab.data(), (size_t)n * sizeof(StepParams), hipMemcpyHostToDevice,
                       s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "hwy_step_group_prepare");
  plan->n = n;
  plan->blocks = blocks;
  plan->big = hwy_step_big(total);
  return HWY_OK;
}

int hwy_step_group(const hwy_step_group_plan* plan, const void* table, void* stream) {
  if (!plan || !table || plan->n < 1 || plan->blocks < 1)
    return fail(HWY_EINVAL, "hwy_step_group: empty plan or NULL table");
  return launched(hwy_launch_step_group((const StepParams*)table, plan->n, plan->blocks,
                                        plan->big, (hipStream_t)stream),
                  "hwy_step_grp_kernel");
}

int64_t hwy_step_group_info_table_bytes(int n) {
  return n < 1 ? -1 : (int64_t)n * (int64_t)sizeof(InfoParams);
}

int hwy_step_group_info_prepare(hwy_handle* const* handles, const hwy_step_io* io,
                                const hwy_step_info* info, int n, void* table, void* info_table,
                                hwy_step_group_plan* plan, void* stream) {
  if (!info || !info_table || n < 1)
    return fail(HWY_EINVAL, "hwy_step_group_info_prepare: info/info_table NULL or n < 1");
  for (int i = 0; i < n; ++i)
    if (int rc = check_info(info + i, "hwy_step_group_info_prepare")) return rc;
  if (int rc = hwy_step_group_prepare(handles, io, n, table, plan, stream)) return rc;
  return upload_table(info_table, info, (size_t)n * sizeof(InfoParams), stream,
                      "hwy_step_group_info_prepare");
}

int hwy_step_group_info(const hwy_step_group_plan* plan, const void* table, const void* info_table,
                        void* stream) {
  if (!plan || !table || !info_table || plan->n < 1 || plan->blocks < 1)
    return fail(HWY_EINVAL, "hwy_step_group_info: empty plan or NULL table");
  return launched(hwy_launch_step_group_info((const StepParams*)table,
                                             (const InfoParams*)info_table, plan->n,
                                             plan->blocks, plan->big, (hipStream_t)stream),
                  "hwy_step_grp_info_kernel");
}

// hwy_step_with_final / hwy_step_group_final_prepare: every refusal before any device call
static int check_final(const hwy_step_info* info, const float* final_obs, const float* obs,
                       const char* who) {
  if (!final_obs) return fail(HWY_EINVAL, "%s: final_obs is NULL", who);
  if (final_obs == obs) return fail(HWY_EINVAL, "%s: final_obs must not be the obs buffer", who);
  return check_ep_stats(info, who);
}

int hwy_step_with_final(hwy_handle* h, const float* actions, float* obs, float* reward,
                        uint8_t* terminated, uint8_t* truncated, float* ep_return,
                        int32_t* ep_length, const hwy_step_info* info, float* final_obs,
                        void* stream) {
  if (!h) return fail(HWY_EINVAL, "handle is NULL");
  const hwy_step_io io = {actions, obs, reward, terminated, truncated, ep_return, ep_length};
  if (int rc = check_step_io("hwy_step_with_final", io)) return rc;
  if (int rc = check_final(info, final_obs, obs, "hwy_step_with_final")) return rc;
  if (int rc = check_pe(h, "hwy_step_with_final")) return rc;
  const StepParams p = step_params(h, io);
  FinalParams f;
  memset(&f, 0, sizeof(f));
  if (info) f.info = *info;
  f.final_obs = final_obs;
  return launched(hwy_launch_step_final(&p, &f, (hipStream_t)stream), "hwy_step_final_kernel");
}

int64_t hwy_step_group_final_table_bytes(int n) {
  return n < 1 ? -1 : (int64_t)n * (int64_t)sizeof(FinalParams);
}

int hwy_step_group_final_prepare(hwy_handle* const* handles, const hwy_step_io* io,
                                 const hwy_step_info* info, float* const* final_obs, int n,
                                 void* table, void* final_table, hwy_step_group_plan* plan,
                                 void* stream) {
  if (!io || !final_obs || !final_table || n < 1)
    return fail(HWY_EINVAL,
                "hwy_step_group_final_prepare: io/final_obs/final_table NULL or n < 1");
  for (int i = 0; i < n; ++i)
    if (int rc = check_final(info ? info + i : nullptr, final_obs[i], io[i].obs,
                             "hwy_step_group_final_prepare"))
      return rc;
  std::vector<FinalParams> ftab(n);  // value-initialised: zero bytes in the padding too
  for (int i = 0; i < n; ++i) {
    if (info) ftab[i].info = info[i];
    ftab[i].final_obs = final_obs[i];
  }
  if (int rc = hwy_step_group_prepare(handles, io, n, table, plan, stream)) return rc;
  return upload_table(final_table, ftab.data(), (size_t)n * sizeof(FinalParams), stream,
                      "hwy_step_group_final_prepare");
}

int hwy_step_group_final(const hwy_step_group_plan* plan, const void* table,
                         const void* final_table, void* stream) {
  if (!plan || !table || !final_table || plan->n < 1 || plan->blocks < 1)
    return fail(HWY_EINVAL, "hwy_step_group_final: empty plan or NULL table");
  return launched(hwy_launch_step_group_final((const StepParams*)table,
                                              (const FinalParams*)final_table, plan->n,
                                              plan->blocks, plan->big, (hipStream_t)stream),
                  "hwy_step_grp_final_kernel");
}

int hwy_export_state(hwy_handle* h, uint32_t* dst, void* stream) {
  if (!h || !dst) return fail(HWY_EINVAL, "handle/dst is NULL");
  hipError_t e =
      hipMemcpyAsync(dst, h->state, state_bytes(h), hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? HWY_OK : hip_fail(e, "hwy_export_state");
}

int hwy_import_state(hwy_handle* h, const uint32_t* src, void* stream) {
  if (!h || !src) return fail(HWY_EINVAL, "handle/src is NULL");
  hipError_t e =
      hipMemcpyAsync(h->state, src, state_bytes(h), hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? HWY_OK : hip_fail(e, "hwy_import_state");
}

int hwy_render_args_size(void) { return (int)sizeof(hwy_render_args); }

// hwy_render's checks that need no handle; on failure the message is set and -1 returned
static int64_t render_bytes(const hwy_render_args* a) {
  if (!a) return fail(HWY_EINVAL, "hwy_render: args is NULL");
  if (a->width < 1 || a->width > 4096 || a->height < 1 || a->height > 4096)
    return fail(HWY_EINVAL, "hwy_render: width and height must be in [1, 4096], got %d x %d",
                a->width, a->height);
  if (a->channels != 1 && a->channels != 3)
    return fail(HWY_EINVAL, "hwy_render: channels must be 1 or 3, got %d", a->channels);
  if (a->n < 1 || a->n > (1 << 22))
    return fail(HWY_EINVAL, "hwy_render: n must be in [1, 2^22], got %d", a->n);
  const float inf = __builtin_inff();
  if (!finite_pos(a->scaling))
    return fail(HWY_EINVAL, "hwy_render: scaling must be finite and > 0");
  for (int i = 0; i < 2; ++i)
    if (!(a->centering[i] > -inf && a->centering[i] < inf))
      return fail(HWY_EINVAL, "hwy_render: centering must be finite");
  if (!a->frames || ((uintptr_t)a->frames & 15u))
    return fail(HWY_EINVAL, "hwy_render: frames must be a 16-byte aligned device pointer");
  return (int64_t)a->n * a->height * a->width * a->channels;
}

int64_t hwy_render_frame_bytes(const hwy_render_args* a) { return render_bytes(a); }

int hwy_render(hwy_handle* h, const hwy_render_args* a, void* stream) {
  if (!h) return fail(HWY_EINVAL, "hwy_render: handle is NULL");
  if (render_bytes(a) < 0) return HWY_EINVAL;
  if (!a->env_ids && a->n > h->cfg.num_envs)
    return fail(HWY_EINVAL, "hwy_render: n = %d frames of a handle of %d envs need env_ids", a->n,
                h->cfg.num_envs);
  RenderParams p;
  p.a = *a;
  p.state = h->state;
  p.num_envs = h->cfg.num_envs;
  p.lanes_count = h->cfg.lanes_count;
  return launched(hwy_launch_render(&p, (hipStream_t)stream), "hwy_render_kernel");
}

int hwy_observe_args_size(void) { return (int)sizeof(hwy_observe_args); }

// hwy_observe_args' and hwy_sense_args' row order
static int check_order(const char* who, int order) {
  if (order != -1 && order != HWY_ORDER_SORTED && order != HWY_ORDER_SHUFFLED)
    return fail(HWY_EINVAL, "%s: order must be -1 (the handle's), sorted or shuffled, got %d", who,
                order);
  return HWY_OK;
}

int hwy_observe_check(const hwy_observe_args* a) {
  if (!a) return fail(HWY_EINVAL, "hwy_observe: args is NULL");
  if (int rc = check_order("hwy_observe", a->order)) return rc;
  if (!a->obs && !a->row_vehicle && !a->veh_values)
    return fail(HWY_EINVAL, "hwy_observe: obs, row_vehicle and veh_values are all NULL");
  if ((a->row_values != nullptr) != (a->veh_values != nullptr))
    return fail(HWY_EINVAL, "hwy_observe: row_values and veh_values go together");
  return HWY_OK;
}

int hwy_observe(hwy_handle* h, const hwy_observe_args* a, void* stream) {
  if (!h) return fail(HWY_EINVAL, "hwy_observe: handle is NULL");
  if (int rc = hwy_observe_check(a)) return rc;
  if (int rc = check_pe(h, "hwy_observe")) return rc;
  ObserveParams p;
  memset(&p, 0, sizeof(p));
  p.p = params_of(h);
  if (a->order >= 0) p.p.cfg.order = a->order;
  p.p.obs = a->obs;
  p.row_vehicle = a->row_vehicle;
  p.row_values = a->row_values;
  p.veh_values = a->veh_values;
  return launched(hwy_launch_observe(&p, (hipStream_t)stream), "hwy_observe_kernel");
}

int hwy_grid_args_size(void) { return (int)sizeof(hwy_grid_args); }

static bool finite_f(float x) { return x > -__builtin_inff() && x < __builtin_inff(); }

int hwy_grid_check(const hwy_grid_args* a) {
  if (!a) return fail(HWY_EINVAL, "hwy_grid: args is NULL");
  if (!a->grid && !a->cell_vehicle && !a->veh_cell && !a->counts)
    return fail(HWY_EINVAL, "hwy_grid: no output given (grid, cell_vehicle, veh_cell and counts "
                            "are all NULL)");
  if (a->nx < 1 || a->ny < 1 || a->nx > HWY_GRID_MAX_CELLS || a->ny > HWY_GRID_MAX_CELLS ||
      a->nx * a->ny > HWY_GRID_MAX_CELLS)
    return fail(HWY_EINVAL, "hwy_grid: nx and ny must be >= 1 with nx * ny <= %d, got %d x %d",
                HWY_GRID_MAX_CELLS, a->nx, a->ny);
  if (!finite_f(a->x0) || !finite_f(a->y0))
    return fail(HWY_EINVAL, "hwy_grid: x0 and y0 must be finite, got %g, %g", (double)a->x0,
                (double)a->y0);
  if (!finite_pos(a->step_x) || !finite_pos(a->step_y))
    return fail(HWY_EINVAL, "hwy_grid: step_x and step_y must be finite and > 0, got %g, %g",
                (double)a->step_x, (double)a->step_y);
  if (a->n_layers < 1 || a->n_layers > HWY_GRID_MAX_LAYERS)
    return fail(HWY_EINVAL, "hwy_grid: n_layers must lie in 1..%d, got %d", HWY_GRID_MAX_LAYERS,
                a->n_layers);
  for (int l = 0; l < a->n_layers; ++l) {
    if (a->layer_ids[l] < 0 || a->layer_ids[l] > HWY_GRID_ON_ROAD)
      return fail(HWY_EINVAL, "hwy_grid: layer_ids[%d] must lie in 0..%d, got %d", l,
                  HWY_GRID_ON_ROAD, a->layer_ids[l]);
    for (int m = 0; m < l; ++m)
      if (a->layer_ids[m] == a->layer_ids[l])
        return fail(HWY_EINVAL, "hwy_grid: layer id %d is given twice (layers %d and %d)",
                    a->layer_ids[l], m, l);
    if (a->has_range[l] && (!finite_f(a->range[l][0]) || !finite_f(a->range[l][1]) ||
                            a->range[l][0] == a->range[l][1]))
      return fail(HWY_EINVAL, "hwy_grid: range[%d] must be finite with lo != hi, got [%g, %g]", l,
                  (double)a->range[l][0], (double)a->range[l][1]);
  }
  const int cells = a->n_layers * a->nx * a->ny + (a->ego_tail ? 1 : 0);
  if (a->row_stride < cells || a->row_stride > HWY_GRID_MAX_STRIDE)
    return fail(HWY_EINVAL, "hwy_grid: row_stride must hold the %d layers of %d x %d%s and be <= "
                            "%d, got %d", a->n_layers, a->nx, a->ny,
                a->ego_tail ? " and the ego tail" : "", HWY_GRID_MAX_STRIDE, a->row_stride);
  return HWY_OK;
}

int hwy_grid(hwy_handle* h, const hwy_grid_args* a, void* stream) {
  if (!h) return fail(HWY_EINVAL, "hwy_grid: handle is NULL");
  if (int rc = hwy_grid_check(a)) return rc;
  GridParams p;
  memset(&p, 0, sizeof(p));
  p.a = *a;
  p.state = h->state;
  p.cfg = h->cfg;
  const int width = a->n_layers * a->nx * a->ny + (a->ego_tail ? h->cfg.n_features : 0);
  if (a->row_stride < width)
    return fail(HWY_EINVAL, "hwy_grid: row_stride %d is below the width %d (%d layers of %d x %d "
                            "and an ego tail of %d)", a->row_stride, width, a->n_layers, a->nx,
                a->ny, h->cfg.n_features);
  return launched(hwy_launch_grid(&p, (hipStream_t)stream), "hwy_grid_kernel");
}

int hwy_lidar_args_size(void) { return (int)sizeof(hwy_lidar_args); }

int hwy_lidar_check(const hwy_lidar_args* a) {
  if (!a) return fail(HWY_EINVAL, "hwy_lidar: args is NULL");
  if (!a->obs && !a->hit_vehicle && !a->seen && !a->counts)
    return fail(HWY_EINVAL, "hwy_lidar: no output given (obs, hit_vehicle, seen and counts are "
                            "all NULL)");
  if (a->cells < 1 || a->cells > HWY_LIDAR_MAX_CELLS)
    return fail(HWY_EINVAL, "hwy_lidar: cells must lie in 1..%d, got %d", HWY_LIDAR_MAX_CELLS,
                a->cells);
  if (a->sub < 1 || a->sub > HWY_LIDAR_MAX_SUB)
    return fail(HWY_EINVAL, "hwy_lidar: sub must lie in 1..%d, got %d", HWY_LIDAR_MAX_SUB, a->sub);
  if (a->cells * a->sub > HWY_LIDAR_MAX_RAYS)
    return fail(HWY_EINVAL, "hwy_lidar: cells * sub must be <= %d, got %d x %d",
                HWY_LIDAR_MAX_RAYS, a->cells, a->sub);
  if (!finite_pos(a->range_m) || !finite_pos(a->speed_scale))
    return fail(HWY_EINVAL, "hwy_lidar: range_m and speed_scale must be finite and > 0, got %g, %g",
                (double)a->range_m, (double)a->speed_scale);
  if (!(a->p_drop >= 0.0f && a->p_drop <= 1.0f))
    return fail(HWY_EINVAL, "hwy_lidar: p_drop must lie in [0, 1], got %g", (double)a->p_drop);
  if (!(a->sigma_r >= 0.0f && a->sigma_r < __builtin_inff()))
    return fail(HWY_EINVAL, "hwy_lidar: sigma_r must be finite and >= 0, got %g",
                (double)a->sigma_r);
  if (a->salt < 0 || a->salt > 65535)
    return fail(HWY_EINVAL, "hwy_lidar: salt must lie in 0..65535, got %d", a->salt);
  const int width = 2 * a->cells + (a->ego_tail ? 1 : 0);
  if (a->row_stride < width || a->row_stride > HWY_LIDAR_MAX_STRIDE)
    return fail(HWY_EINVAL, "hwy_lidar: row_stride must hold the %d cells%s and be <= %d, got %d",
                a->cells, a->ego_tail ? " and the ego tail" : "", HWY_LIDAR_MAX_STRIDE,
                a->row_stride);
  return HWY_OK;
}

int hwy_lidar(hwy_handle* h, const hwy_lidar_args* a, void* stream) {
  if (!h) return fail(HWY_EINVAL, "hwy_lidar: handle is NULL");
  if (int rc = hwy_lidar_check(a)) return rc;
  LidarParams p;
  memset(&p, 0, sizeof(p));
  p.a = *a;
  p.state = h->state;
  p.cfg = h->cfg;
  p.dth = (float)(6.283185307179586 / (double)(a->cells * a->sub));
  p.salt_word = HWY_LIDAR_SALT + (uint32_t)a->salt;
  // 4 m over the 2.7 m half diagonal, and 1e-4 of the range over what binary32 rounds of it
  const float far = (a->range_m + 4.0f) * 1.0001f;
  p.cull2 = far * far;  // +inf for a range near FLT_MAX: nothing is culled
  const int width = 2 * a->cells + (a->ego_tail ? h->cfg.n_features : 0);
  if (a->row_stride < width)
    return fail(HWY_EINVAL, "hwy_lidar: row_stride %d is below the width %d (%d cells and an ego "
                            "tail of %d)", a->row_stride, width, a->cells, h->cfg.n_features);
  return launched(hwy_launch_lidar(&p, (hipStream_t)stream), "hwy_lidar_kernel");
}

int hwy_traffic_args_size(void) { return (int)sizeof(hwy_traffic_args); }

int hwy_traffic_check(const hwy_traffic_args* a) {
  if (!a) return fail(HWY_EINVAL, "hwy_traffic: args is NULL");
  if (!a->front && !a->rear && !a->gap && !a->closing && !a->ttc && !a->thw && !a->risk &&
      !a->ego && !a->acc)
    return fail(HWY_EINVAL, "hwy_traffic: no output given (front, rear, gap, closing, ttc, thw, "
                            "risk, ego and acc are all NULL)");
  if (a->ep_stats && !a->acc) return fail(HWY_EINVAL, "hwy_traffic: ep_stats needs acc");
  for (int k = 0; k < 3; ++k)
    if (a->restart[k] && !a->acc)
      return fail(HWY_EINVAL, "hwy_traffic: restart[%d] needs acc", k);
  const float vals[4] = {a->ttc_thresh, a->thw_thresh, a->risk_horizon, a->near_range};
  const char* names[4] = {"ttc_thresh", "thw_thresh", "risk_horizon", "near_range"};
  for (int i = 0; i < 4; ++i)
    if (!finite_pos(vals[i]))
      return fail(HWY_EINVAL, "hwy_traffic: %s must be finite and > 0, got %g", names[i],
                  (double)vals[i]);
  return HWY_OK;
}

int hwy_traffic(hwy_handle* h, const hwy_traffic_args* a, void* stream) {
  if (!h) return fail(HWY_EINVAL, "hwy_traffic: handle is NULL");
  if (int rc = hwy_traffic_check(a)) return rc;
  TrafficParams p;
  p.a = *a;
  p.state = h->state;
  p.cfg = h->cfg;
  return launched(hwy_launch_traffic(&p, (hipStream_t)stream), "hwy_traffic_kernel");
}

int hwy_sense_args_size(void) { return (int)sizeof(hwy_sense_args); }

int hwy_sense_check(const hwy_sense_args* a) {
  if (!a) return fail(HWY_EINVAL, "hwy_sense: args is NULL");
  if (int rc = check_order("hwy_sense", a->order)) return rc;
  const float inf = __builtin_inff();
  if (!(a->range_m > 0.0f))  // +inf passes, a NaN does not
    return fail(HWY_EINVAL, "hwy_sense: range_m must be > 0 (+inf: no range limit), got %g",
                (double)a->range_m);
  if (!(a->p_drop >= 0.0f && a->p_drop <= 1.0f))
    return fail(HWY_EINVAL, "hwy_sense: p_drop must lie in [0, 1], got %g", (double)a->p_drop);
  for (int c = 0; c < 3; ++c)
    if (!(a->sigma[c] >= 0.0f && a->sigma[c] < inf))
      return fail(HWY_EINVAL, "hwy_sense: sigma[%d] must be finite and >= 0, got %g", c,
                  (double)a->sigma[c]);
  if (a->salt < 0 || a->salt > 65535)
    return fail(HWY_EINVAL, "hwy_sense: salt must lie in 0..65535, got %d", a->salt);
  if (!a->obs && !a->row_vehicle && !a->visible && !a->hidden && !a->counts)
    return fail(HWY_EINVAL, "hwy_sense: no output given (obs, row_vehicle, visible, hidden and "
                            "counts are all NULL)");
  return HWY_OK;
}

int hwy_sense(hwy_handle* h, const hwy_sense_args* a, void* stream) {
  if (!h) return fail(HWY_EINVAL, "hwy_sense: handle is NULL");
  if (int rc = hwy_sense_check(a)) return rc;
  if (int rc = check_pe(h, "hwy_sense")) return rc;
  SenseParams p;
  memset(&p, 0, sizeof(p));
  p.p = params_of(h);
  if (a->order >= 0) p.p.cfg.order = a->order;
  p.p.obs = a->obs;
  p.a = *a;
  p.salt_word = HWY_SENSE_SALT + (uint32_t)a->salt;
  p.range2 = a->range_m * a->range_m;
  // 4 m over the 2.7 m half diagonal, and 1e-4 of the range over what binary32 rounds of it
  const float far = (a->range_m + 4.0f) * 1.0001f;
  p.cull2 = far * far;
  return launched(hwy_launch_sense(&p, (hipStream_t)stream), "hwy_sense_kernel");
}

int hwy_lookahead_args_size(void) { return (int)sizeof(hwy_lookahead_args); }

int hwy_lookahead_check(const hwy_lookahead_args* a) {
  if (!a) return fail(HWY_EINVAL, "hwy_lookahead: args is NULL");
  if (a->k < 1 || a->k > HWY_LOOKAHEAD_MAX_K)
    return fail(HWY_EINVAL, "hwy_lookahead: k must lie in 1..%d, got %d", HWY_LOOKAHEAD_MAX_K, a->k);
  if (a->horizon < 1 || a->horizon > HWY_LOOKAHEAD_MAX_H)
    return fail(HWY_EINVAL, "hwy_lookahead: horizon must lie in 1..%d, got %d",
                HWY_LOOKAHEAD_MAX_H, a->horizon);
  if (!(a->gamma >= 0.0f && a->gamma <= 1.0f))  // a NaN fails both
    return fail(HWY_EINVAL, "hwy_lookahead: gamma must be finite and lie in [0, 1], got %g",
                (double)a->gamma);
  if (!a->actions) return fail(HWY_EINVAL, "hwy_lookahead: actions is NULL");
  if (!a->steps && !a->terminated && !a->truncated && !a->rewards && !a->ret && !a->ego_final &&
      !a->obs && !a->chosen && !a->chosen_action)
    return fail(HWY_EINVAL, "hwy_lookahead: no output given");
  if ((a->lazy || a->chosen) && !(a->steps && a->terminated))
    return fail(HWY_EINVAL, "hwy_lookahead: lazy and chosen need steps and terminated");
  if (a->chosen_action && !a->chosen)
    return fail(HWY_EINVAL, "hwy_lookahead: chosen_action needs chosen");
  return HWY_OK;
}

int hwy_lookahead(hwy_handle* h, const hwy_lookahead_args* a, void* stream) {
  if (!h) return fail(HWY_EINVAL, "hwy_lookahead: handle is NULL");
  if (int rc = hwy_lookahead_check(a)) return rc;
  if ((int64_t)h->cfg.num_envs * a->k > HWY_LOOKAHEAD_MAX_BRANCHES)
    return fail(HWY_EINVAL, "hwy_lookahead: num_envs * k must be <= %d, got %d * %d",
                HWY_LOOKAHEAD_MAX_BRANCHES, h->cfg.num_envs, a->k);
  if (a->obs)
    if (int rc = check_pe(h, "hwy_lookahead")) return rc;
  LookaheadParams p;
  memset(&p, 0, sizeof(p));
  p.p = params_of(h);
  p.a = *a;
  hipStream_t s = (hipStream_t)stream;
  const int E = h->cfg.num_envs;
  if (a->lazy && a->k > 1) {
    // candidate 0 of every env, then the rest behind it on the stream, each wave gated by its
    // env's terminated[e][0]
    p.k0 = 0, p.nk = 1, p.gate = 0;
    if (hwy_launch_lookahead(&p, hwy_step_big(E), s))
      return hip_fail(hipGetLastError(), "hwy_lookahead_kernel");
    p.k0 = 1, p.nk = a->k - 1, p.gate = 1;
    if (hwy_launch_lookahead(&p, hwy_step_big((int64_t)E * p.nk), s))
      return hip_fail(hipGetLastError(), "hwy_lookahead_kernel");
  } else {
    p.k0 = 0, p.nk = a->k, p.gate = 0;
    if (hwy_launch_lookahead(&p, hwy_step_big((int64_t)E * p.nk), s))
      return hip_fail(hipGetLastError(), "hwy_lookahead_kernel");
  }
  if (a->chosen && hwy_launch_lookahead_choice(&p, s))
    return hip_fail(hipGetLastError(), "hwy_lookahead_choice_kernel");
  return HWY_OK;
}

int hwy_obs_pe(const float* obs_in, float* obs_out, int E, int N, int F, int kind, int d,
               int ego_idx, float max_dist, const float* table, const float* dist_override,
               void* stream) {
  if (E < 0 || N < 1 || F < 1 || F > HWY_MAX_FEATURES)
    return fail(HWY_EINVAL, "hwy_obs_pe: bad shape E=%d N=%d F=%d", E, N, F);
  if (kind == HWY_PE_ROPE && (d % 2 || d > F || d < 0))
    return fail(HWY_EINVAL, "rotate_dim must be even and <= %d; got %d", F, d);
  if ((kind == HWY_PE_DIST || kind == HWY_PE_DIST1) && (d % 2 || d < 2))
    return fail(HWY_EINVAL, "DistanceEmbedWrapper requires even d_embed; got %d", d);
  if ((kind == HWY_PE_DIST || kind == HWY_PE_ROPE) && F < 2)
    return fail(HWY_EINVAL, "distance wrappers need at least 2 features");
  if (kind < HWY_PE_NONE || kind > HWY_PE_DIST1) return fail(HWY_EINVAL, "unknown pe kind %d", kind);
  if (ego_idx < 0 || ego_idx >= N) return fail(HWY_EINVAL, "ego_idx %d out of range", ego_idx);
  if (kind != HWY_PE_NONE && !table && !(kind == HWY_PE_ROPE && d == 0))
    return fail(HWY_EINVAL, "pe table is NULL");
  return launched(hwy_launch_obs_pe(obs_in, obs_out, E, N, F, kind, d, ego_idx, max_dist, table,
                                    dist_override, (hipStream_t)stream),
                  "hwy_obs_pe_kernel");
}

int hwy_gae(const float* rewards, const uint8_t* dones, const float* values,
            const float* last_values, double gamma, double lam, int T, int E, float* advantages,
            float* returns, void* stream) {
  if (T < 0 || E < 0) return fail(HWY_EINVAL, "hwy_gae: bad shape T=%d E=%d", T, E);
  if (T == 0 || E == 0) return HWY_OK;
  return launched(hwy_launch_gae(rewards, dones, values, last_values, gamma, lam, T, E,
                                 advantages, returns, (hipStream_t)stream),
                  "hwy_gae_kernel");
}

int hwy_gae_boot(const float* rewards, const uint8_t* terminated, const uint8_t* truncated,
                 const float* values, const float* last_values, const float* boot_values,
                 double gamma, double lam, int T, int E, float* advantages, float* returns,
                 void* stream) {
  if (T < 0 || E < 0) return fail(HWY_EINVAL, "hwy_gae_boot: bad shape T=%d E=%d", T, E);
  if (T == 0 || E == 0) return HWY_OK;
  return launched(hwy_launch_gae_boot(rewards, terminated, truncated, values, last_values,
                                      boot_values, gamma, lam, T, E, advantages, returns,
                                      (hipStream_t)stream),
                  "hwy_gae_boot_kernel");
}

int hwy_math_selftest(int op, const float* in, const float* in2, float* out, int n, void* stream) {
  if (op < 0 || op > 16 || n < 0) return fail(HWY_EINVAL, "bad selftest op %d", op);
  return launched(hwy_launch_math(op, in, in2, out, n, (hipStream_t)stream), "hwy_math_kernel");
}

}  // extern "C"
