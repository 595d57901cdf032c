// hwy_kernels.hip -- gfx950 kernels of the vectorised highway-v0 hot path.
//
// Layout: one 64-lane wavefront per env, lane v = vehicle v of road.vehicles (v = 0 ego,
// 1..vehicles_count IDM traffic).  A 256-thread workgroup advances 4 envs.  The per-env state is
// field-major SoA in HBM ([field][env][64] u32, include/hwy.h) so each wave loads 256
// contiguous bytes per field once, runs all sim_freq/policy_freq frames in registers, and
// stores once.  Cross-vehicle reads use v_readlane (uniform index, SGPR broadcast) or
// ds_bpermute (per-lane index); nothing else touches LDS except the observation row maps.
//
// Semantics follow upstream highway-env 1.10.1 as restated in oracle/hwy_oracle.c, which runs
// every vehicle sequentially; the parallel formulation below is arranged to give the same bits:
//   * Road.act order dependence: MOBIL decisions do not read other vehicles' target lanes, so
//     they run in parallel; the "abort ongoing lane change" check (which does) runs afterwards
//     over the mid-change vehicles in ascending index, each seeing the already-final targets of
//     lower-index vehicles and the frame-start targets of higher-index ones.
//   * Road.step collisions: lane k evaluates every pair {k, j} (always as a = lower index, so
//     both lanes of a pair compute identical bits) in ascending j, which is exactly the order
//     in which upstream's i<j double loop last writes k's impact.
// All floating point goes through hwy_math.h and is compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hwy.h"
#include "hwy_math.h"
#include "hwy_internal.h"

#define WAVE 64
// envs (one wave each) per workgroup: 1, 2 and 4 measured the same (round 4)
constexpr int ENVS_PER_BLOCK = 4;

// upstream constants (same literals as oracle/hwy_oracle.c)
#define LANE_WIDTH 4.0f
#define LANE_VEH_LEN 5.0f
#define ROAD_LENGTH 10000.0f
#define VEH_LENGTH 5.0f
#define VEH_WIDTH 2.0f
#define MAX_SPEED 40.0f
#define MIN_SPEED (-40.0f)
#define KP_HEADING (1.0f / 0.2f)
#define KP_LATERAL (1.0f / 0.6f)
#define MAX_STEERING (HM_PI_F / 3.0f)
#define TAN_MAX_STEERING 1.7320509f  // tan(MAX_STEERING), correctly rounded
#define ACC_MAX 6.0f
#define COMFORT_ACC_MAX 3.0f
#define DISTANCE_WANTED 10.0f
#define TIME_WANTED 1.5f
#define LANE_CHANGE_MIN_ACC_GAIN 0.2f
#define LANE_CHANGE_MAX_BRAKING_IMPOSED 2.0f
#define LANE_CHANGE_DELAY 1.0f
#define PERCEPTION_DISTANCE 200.0f
#define TWO_SQRT_AB 7.745966692414834f
#define INV_TWO_SQRT_AB 0.12909944487358056f  // 1 / (2 sqrt(15)), correctly rounded
#define VEH_DIAGONAL 5.385164807134504f

// ------------------------------------------------------------------------- wave primitives
__device__ __forceinline__ float rdlf(float v, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}
__device__ __forceinline__ int rdli(int v, int k) { return __builtin_amdgcn_readlane(v, k); }
// per-lane gather; must run with all 64 lanes active
__device__ __forceinline__ float shf(float v, int src) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v)));
}
__device__ __forceinline__ int shi(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }
// DPP forms (VALU-local, no LDS round trip); all 64 lanes active.  GFX9 DPP controls:
// wave_shr:1 0x138, row_shr:k 0x110+k, row_bcast:15 0x142, row_bcast:31 0x143,
// quad_perm 0x00-0xFF, row_mirror 0x140, row_half_mirror 0x141.
// lane i <- lane i-1; lane 0 keeps its own value
__device__ __forceinline__ float shr1f(float v) {
  const int b = __float_as_int(v);
  return __int_as_float(__builtin_amdgcn_update_dpp(b, b, 0x138, 0xf, 0xf, false));
}
// lane i <- lane i+1; lane 63 keeps its own value
__device__ __forceinline__ int shl1i(int v) {
  return __builtin_amdgcn_update_dpp(v, v, 0x130, 0xf, 0xf, false);
}
__device__ __forceinline__ int shr1i(int v) {
  return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false);
}
// lane i <- lane i^1
__device__ __forceinline__ int swp1i(int v) {
  return __builtin_amdgcn_update_dpp(v, v, 0xb1, 0xf, 0xf, false);
}
// inclusive prefix sum over the 64 lanes
__device__ __forceinline__ int wave_incl_scan(int x) {
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
  return x;
}
// max over the 64 lanes (exact: no NaN reaches it), uniform result
__device__ __forceinline__ float wave_max_f(float v) {
  int b = __float_as_int(v);
  b = __float_as_int(hm_maxf(__int_as_float(b), __int_as_float(
      __builtin_amdgcn_update_dpp(b, b, 0xb1, 0xf, 0xf, false))));
  b = __float_as_int(hm_maxf(__int_as_float(b), __int_as_float(
      __builtin_amdgcn_update_dpp(b, b, 0x4e, 0xf, 0xf, false))));
  b = __float_as_int(hm_maxf(__int_as_float(b), __int_as_float(
      __builtin_amdgcn_update_dpp(b, b, 0x141, 0xf, 0xf, false))));
  b = __float_as_int(hm_maxf(__int_as_float(b), __int_as_float(
      __builtin_amdgcn_update_dpp(b, b, 0x140, 0xf, 0xf, false))));
  b = __float_as_int(hm_maxf(__int_as_float(b), __int_as_float(
      __builtin_amdgcn_update_dpp(b, b, 0x142, 0xa, 0xf, false))));
  b = __float_as_int(hm_maxf(__int_as_float(b), __int_as_float(
      __builtin_amdgcn_update_dpp(b, b, 0x143, 0xc, 0xf, false))));
  return __int_as_float(__builtin_amdgcn_readlane(b, 63));
}
// the lane mask of p straight from the compare (HIP's __ballot(int) re-materialises p as an
// int and compares it again: two VALU per ballot)
__device__ __forceinline__ uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool wave_any(bool p) { return ballot(p) != 0ull; }
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------- section clocks
// Development build only (make prof -> libhwy_prof.so): per-section shader-clock totals of the
// step kernel, accumulated per env (plain loads and stores by the env's own wave: one device
// atomic per section and wave on shared counters serialised the launch's tail and inflated the
// last sections several-fold) and summed over envs by hwy_debug_sections().
#define HWY_NSEC 18
#define HWY_NSEC_ENVS 32768  // the largest profiled workload (configs[4]: 32,768 envs per GPU)
#ifdef HWY_SECTION_PROFILE
__device__ unsigned long long g_hwy_sections[HWY_NSEC_ENVS][HWY_NSEC];
struct SecProf {
  uint64_t t;
  uint64_t acc[HWY_NSEC];
};
#define SEC_START(sp)                                      \
  do {                                                     \
    (sp).t = __builtin_amdgcn_s_memtime();                 \
    for (int _i = 0; _i < HWY_NSEC; ++_i) (sp).acc[_i] = 0; \
  } while (0)
#define SEC(sp, id)                                      \
  do {                                                   \
    const uint64_t _n = __builtin_amdgcn_s_memtime();    \
    (sp).acc[id] += _n - (sp).t;                         \
    (sp).t = _n;                                         \
  } while (0)
#define SEC_FLUSH(sp, lane, e)                                                \
  do {                                                                        \
    if ((lane) == 0) /* envs past the cap fold onto env mod cap: none is dropped */ \
      for (int _i = 0; _i < HWY_NSEC; ++_i)                                   \
        g_hwy_sections[(e) % HWY_NSEC_ENVS][_i] += (sp).acc[_i];             \
  } while (0)
#else
struct SecProf {};
#define SEC_START(sp) \
  do {                \
  } while (0)
#define SEC(sp, id) \
  do {              \
  } while (0)
#define SEC_FLUSH(sp, lane, e) \
  do {                         \
  } while (0)
#endif
// Development builds (make prof / make waves -> libhwy_waves.so, tools/probe_waves.py):
#if defined(HWY_SECTION_PROFILE) || defined(HWY_WAVE_TIMES)
// per-env (start, end, done | HW_ID << 8 | XCC_ID << 40) of the last step launch, first
// HWY_NWT envs
#define HWY_NWT 16384
__device__ unsigned long long g_hwy_wave_t[5 * HWY_NWT];
#define WAVE_T(e, lane, k, val)                                          \
  do {                                                                   \
    if ((lane) == 0 && (e) < HWY_NWT) g_hwy_wave_t[5 * (e) + (k)] = (val); \
  } while (0)
#define WAVE_HWID()                                                                  \
  (((unsigned long long)(uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 8) |  \
   ((unsigned long long)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xff) << 40))
#else
#define WAVE_T(e, lane, k, val) \
  do {                          \
  } while (0)
#define WAVE_HWID() 0ull
#endif

// Development pricing builds only (hwy_dev_knobs.h, a make variant with -DHWY_DEV_KNOBS and the
// mask; WRONG results, never the product): kSkip skips parts of the frame to price their
// instruction count.  The product build compiles every such site away (kSkip = 0).
#ifdef HWY_DEV_KNOBS
#include "hwy_dev_knobs.h"
#else
constexpr int kSkip = 0;
#endif

// ------------------------------------------------------------------------- vehicle state
struct Veh {
  float x, y, h, spd, tsp, dlt, tmr, ix, iy;
  // Vehicle.action.  asteer: lane 0 the ego's steering angle (persists across frames); the
  // traffic lanes hold the TANGENT of their clipped steering angle (what kinematics uses)
  float aacc, asteer;
  int ln, tl;
  bool crashed, imp, present;
};

__device__ __forceinline__ float lane_lat(float y, int c) { return y - (float)c * LANE_WIDTH; }

__device__ __forceinline__ bool on_lane_m(float x, float y, int c, float margin) {
  float lat = lane_lat(y, c);
  return hm_absf(lat) <= LANE_WIDTH / 2.0f + margin && -LANE_VEH_LEN <= x &&
         x < ROAD_LENGTH + LANE_VEH_LEN;
}

// the loop form: the first lane of least |lateral offset| (upstream's argmin over the lanes)
__device__ __forceinline__ int closest_lane_scan(float y, int lanes) {
  int best = 0;
  float bd = hm_absf(lane_lat(y, 0));
  for (int c = 1; c < lanes; ++c) {
    float d = hm_absf(lane_lat(y, c));
    if (d < bd) {
      bd = d;
      best = c;
    }
  }
  return best;
}

// closest_lane_scan's answer from two candidates: for |y| < 2^20 (lane offsets exact to 1/8) the
// first least offset is c0 = floor(y / 4) clamped to the lanes, or c0 + 1 if its offset is
// strictly smaller.  Below c0 the offsets are >= 4 > |offset(c0)| (y - 4 c0 is exact, Sterbenz),
// above c0 + 1 likewise; outside the road the offsets are strictly monotone in c.  Any other y
// (and NaN) takes the scan.
__device__ __forceinline__ int closest_lane(float y, int lanes) {
  if (!(hm_absf(y) < 1048576.0f)) return closest_lane_scan(y, lanes);
  const float q = hm_floorf(y * (1.0f / LANE_WIDTH));
  const int c0 = q >= (float)(lanes - 1) ? lanes - 1 : (q > 0.0f ? (int)q : 0);
  const bool up = c0 + 1 < lanes && hm_absf(lane_lat(y, c0 + 1)) < hm_absf(lane_lat(y, c0));
  return up ? c0 + 1 : c0;
}

// IDMVehicle.desired_gap(ego=a, front=b), from the velocity vectors (speed * (cos h, sin h),
// formed once per vehicle and frame: the same products upstream's velocity property forms)
__device__ __forceinline__ float desired_gap_v(float a_spd, float a_c, float a_s, float avx,
                                               float avy, float bvx, float bvy) {
  float dv = hm_fma(avx - bvx, a_c, (avy - bvy) * a_s);
  return hm_fma(a_spd, TIME_WANTED, DISTANCE_WANTED) + (a_spd * dv) * INV_TWO_SQRT_AB;
}

// IDMVehicle.acceleration, free-road term: the ego vehicle's base speed / target speed ...
__device__ __forceinline__ float idm_base(float ev_spd, float ev_tsp, float limit) {
  float tsp = hm_clipf(ev_tsp, 0.0f, limit);
  return hm_maxf(ev_spd, 0.0f) / hm_absf(hm_not_zero(tsp));
}

// ... raised to the deciding vehicle's DELTA, from the base and its log (hm_logf_idm):
// np.power(base, DELTA) in hm_powf's arithmetic, branch-free (bit-identical, hwy_math.h)
__device__ __forceinline__ float idm_free_from(float base, float lg, float delta) {
  if (kSkip & 32) return hm_fma(-COMFORT_ACC_MAX, base * base, COMFORT_ACC_MAX);
  return hm_fma(-COMFORT_ACC_MAX, hm_expf_idm(lg, delta, base), COMFORT_ACC_MAX);
}

// IDMVehicle.acceleration given its free-road term `acc` (interaction with the front vehicle)
// (ev_vx, ev_vy, fv_vx, fv_vy: the two velocity vectors)
__device__ __forceinline__ float idm_with_front(float acc, float ev_spd, float ev_x, float ev_c,
                                                float ev_s, float ev_vx, float ev_vy,
                                                bool has_front, float fv_x, float fv_vx,
                                                float fv_vy) {
  if (has_front) {
    float d = fv_x - ev_x;
    float g = desired_gap_v(ev_spd, ev_c, ev_s, ev_vx, ev_vy, fv_vx, fv_vy) / hm_not_zero(d);
    acc = hm_fma(-COMFORT_ACC_MAX, g * g, acc);
  }
  return acc;
}

// ControlledVehicle.steering_control(target lane c) clipped to +-MAX_STEERING, returned as its
// tangent.  Closed form (DESIGN.md deviations; oracle steering_tan): with z the clipped sine of
// the slip angle, tan(clip(atan(2 tan(asin z)))) = clip(2 z / sqrt((1 - z)(1 + z)), +-tan MAX).
__device__ __forceinline__ float steering_tan(float y, float h, float spd, int c) {
  float lat = lane_lat(y, c);
  float lane_future_heading = 0.0f;
  float lateral_speed_command = -KP_LATERAL * lat;
  const float inv_spd = 1.0f / hm_not_zero(spd);  // both of upstream's divisions by not_zero(speed)
  float heading_command = hm_asinf(hm_clipf(lateral_speed_command * inv_spd, -1.0f, 1.0f));
  float heading_ref = lane_future_heading + hm_clipf(heading_command, -HM_PIO4_F, HM_PIO4_F);
  float heading_rate_command = KP_HEADING * hm_wrap_to_pi(heading_ref - h);
  const float z =
      hm_clipf(((VEH_LENGTH / 2.0f) * inv_spd) * heading_rate_command, -1.0f, 1.0f);
  const float t = 2.0f * (z / __builtin_sqrtf((1.0f - z) * (1.0f + z)));
  return hm_clipf(t, -TAN_MAX_STEERING, TAN_MAX_STEERING);
}

// utils.are_polygons_intersecting on the two 5x2 m rectangles (a = lower road index), in the
// closed form of oracle/hwy_oracle.c rect_sat (same operations in the same order): intervals
// centre.n -/+ (L/2 |u.n| + W/2 |v.n|) on upstream's eight edge normals
// -u_a, v_a, u_a, -v_a, -u_b, v_b, u_b, -v_b, the opposite ones by exact negation.
__device__ __forceinline__ void rect_interval(float x, float y, float c, float s, float nx,
                                              float ny, float& mn, float& mx) {
  const float p = hm_fma(x, nx, y * ny);
  const float r = hm_fma(VEH_LENGTH / 2.0f, hm_absf(hm_fma(c, nx, s * ny)),
                         (VEH_WIDTH / 2.0f) * hm_absf(hm_fma(c, ny, -(s * nx))));
  mn = p - r;
  mx = p + r;
}

__device__ __forceinline__ float interval_distance(float min_a, float max_a, float min_b,
                                                   float max_b) {
  return min_a < min_b ? min_b - max_a : min_a - max_b;
}

// `activem`: the lanes holding a pair.  The wave stops once every active lane has broken out
// (nothing changes for a lane after its break), which after a's own two normals is the usual
// case: cars in adjacent lanes separate on v_a, cars in one lane on u_a.  Each edge runs on every
// lane: a lane already out has inter = will = false, which the edge's updates keep (the same
// values upstream's break leaves); the break test reads wave masks kept from the compares.
__device__ __forceinline__ void sat_collide(uint64_t activem, float xa, float ya, float ca, float sa,
                                            float dax, float day, float xb, float yb, float cb,
                                            float sb, float dbx, float dby, bool* inter_out,
                                            bool* will_out, float* tx, float* ty) {
  const float cdx = xa - xb, cdy = ya - yb;
  const float ddx = dax - dbx, ddy = day - dby;
  bool inter = true, will = true;
  uint64_t interm = activem, willm = activem;  // ballot(active && inter), ballot(active && will)
  float min_distance = __builtin_huge_valf(), axx = 0.0f, axy = 0.0f;
  float pa0[2], pa1[2], pb0[2], pb1[2], vpk[2], cdk[2], nxk[2], nyk[2];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = e & 1;
    float min_a, max_a, min_b, max_b, vp, cd, sx, sy;
    if (!(e & 2)) {  // -u (k = 0) or v (k = 1) of rectangle e / 4
      const float c = e < 4 ? ca : cb, s = e < 4 ? sa : sb;
      nxk[k] = k ? -s : -c;
      nyk[k] = k ? c : -s;
      rect_interval(xa, ya, ca, sa, nxk[k], nyk[k], pa0[k], pa1[k]);
      rect_interval(xb, yb, cb, sb, nxk[k], nyk[k], pb0[k], pb1[k]);
      vpk[k] = hm_fma(nxk[k], ddx, nyk[k] * ddy);
      cdk[k] = hm_fma(cdx, nxk[k], cdy * nyk[k]);
      min_a = pa0[k], max_a = pa1[k], min_b = pb0[k], max_b = pb1[k];
      vp = vpk[k], cd = cdk[k], sx = nxk[k], sy = nyk[k];
    } else {  // the opposite edge: n -> -n
      min_a = -pa1[k], max_a = -pa0[k], min_b = -pb1[k], max_b = -pb0[k];
      vp = -vpk[k], cd = -cdk[k], sx = -nxk[k], sy = -nyk[k];
    }
    {  // upstream breaks out once both are false (a lane past that keeps both false here)
      const bool s0 = interval_distance(min_a, max_a, min_b, max_b) > 0.0f;
      inter = inter && !s0;
      if (vp < 0.0f)
        min_a = min_a + vp;
      else
        max_a = max_a + vp;
      const float distance = interval_distance(min_a, max_a, min_b, max_b);
      const bool s1 = distance > 0.0f;
      will = will && !s1;
      interm &= ~ballot(s0);
      willm &= ~ballot(s1);
      if ((inter || will) && hm_absf(distance) < min_distance) {
        min_distance = hm_absf(distance);
        axx = cd > 0.0f ? sx : -sx;
        axy = cd > 0.0f ? sy : -sy;
      }
    }
    if ((e & 1) && e < 7 && !(interm | willm)) break;
  }
  *inter_out = inter;
  *will_out = will;
  *tx = will ? min_distance * axx : 0.0f;
  *ty = will ? min_distance * axy : 0.0f;
}

// ------------------------------------------------------------------------- reset
__device__ __forceinline__ uint64_t schedule_seed(const hwy_config& C, int e, int episode) {
  return (uint64_t)(C.seed_base + (int64_t)C.env_offset + (int64_t)e + 1 +
                    C.seed_stride * (int64_t)episode);
}

// the seed of (env e, episode k): the handle's schedule, or its experiment group's
// (hwy_set_seed_groups: group g = e / group_envs, l = e - g * group_envs)
__device__ __forceinline__ uint64_t episode_seed(const StepParams& P, int e, int episode) {
  const hwy_config& C = P.cfg;
  if (!P.group_seed) return schedule_seed(C, e, episode);
  const int g = e / P.group_envs, l = e - g * P.group_envs;
  return (uint64_t)(P.group_seed[g] + (int64_t)C.env_offset + (int64_t)l + 1 +
                    C.seed_stride * (int64_t)episode);
}

__device__ __forceinline__ const float* group_pe_table(const StepParams& P, int e) {
  return P.pe_group_stride ? P.pe_table + (size_t)(e / P.group_envs) * P.pe_group_stride
                           : P.pe_table;
}

// HighwayEnv._create_vehicles via Vehicle.create_random / IDMVehicle.randomize_behavior
__device__ void reset_wave(const hwy_config& C, int lane, uint64_t seed, Veh& v) {
  const int V = C.vehicles_count + 1;
  const int lanes = C.lanes_count;
  uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
  hm_u32x4 u = hm_philox4x32_10((uint32_t)lane, 0u, 0u, 0x52535431u, k0, k1);
  float fac = hm_expf((-5.0f / 40.0f) * (float)lanes);
  int ln;
  float speed, spacing;
  if (lane == 0) {
    ln = C.initial_lane_id >= 0 ? C.initial_lane_id : hm_choice(u.v[0], lanes);
    speed = 25.0f;
    spacing = C.ego_spacing;
  } else {
    ln = hm_choice(u.v[0], lanes);
    speed = hm_uniform(u.v[1], 0.7f * C.speed_limit, 0.8f * C.speed_limit);
    spacing = 1.0f / C.vehicles_density;
  }
  float default_spacing = 12.0f + 1.0f * speed;
  float offset = spacing * default_spacing * fac;
  float inc = offset * hm_uniform(u.v[2], 0.9f, 1.1f);
  // x0 = max(x of vehicles already on the road) + inc: a sequential chain in road order
  float mx = 3.0f * rdlf(offset, 0) + rdlf(inc, 0);
  float x = mx;
  for (int k = 1; k < V; ++k) {
    float xk = mx + rdlf(inc, k);
    if (lane == k) x = xk;
    if (xk > mx) mx = xk;
  }
  v.x = x;
  v.y = (float)ln * LANE_WIDTH;
  v.h = 0.0f;
  v.spd = speed;
  v.ln = ln;
  v.tl = ln;
  v.tsp = speed;
  v.present = lane < V;
  v.crashed = false;
  v.imp = false;
  v.ix = 0.0f;
  v.iy = 0.0f;
  v.aacc = 0.0f;
  v.asteer = 0.0f;
  if (lane == 0) {
    v.dlt = 0.0f;
    v.tmr = 0.0f;
  } else {
    float t = (v.x + v.y) * HM_PI_F;
    v.tmr = t - hm_floorf(t);
    v.dlt = hm_uniform(u.v[3], 3.5f, 4.5f);
  }
  if (!v.present) {
    v.x = v.y = v.spd = v.tsp = v.dlt = v.tmr = 0.0f;
    v.ln = v.tl = 0;
  }
}

// road-order position of every vehicle after a reset: create_random places each car ahead of all
// previous ones (x strictly increasing with the index), so the order is the index order
__device__ __forceinline__ int reset_order_pos(int lane, int V) {
  return lane < V ? lane : V + (WAVE - 1 - lane);
}

// ------------------------------------------------------------------------- observation
__device__ __forceinline__ float feature_value(int fid, float x, float y, float spd, float h,
                                               float c, float s) {
  switch (fid) {
    case HWY_FEAT_PRESENCE: return 1.0f;
    case HWY_FEAT_X: return x;
    case HWY_FEAT_Y: return y;
    case HWY_FEAT_VX: return spd * c;
    case HWY_FEAT_VY: return spd * s;
    case HWY_FEAT_COS_H: return c;
    case HWY_FEAT_SIN_H: return s;
    case HWY_FEAT_HEADING: return h;
  }
  return 0.0f;
}
__device__ __forceinline__ bool is_relative_feature(int fid) {
  return fid == HWY_FEAT_X || fid == HWY_FEAT_Y || fid == HWY_FEAT_VX || fid == HWY_FEAT_VY;
}

// One wrapped observation row: in[F] (row values), exy = ego row's first two values.
// Writes F_out values to out (global).  rope_embed.py:44-74 / dist_embed.py:76-96 /
// rank_embed.py:45-51.
__device__ __forceinline__ void write_pe_row(const float* vals, int F, int kind, int d, int row,
                                             float ex0, float ex1, float max_dist,
                                             const float* table, bool have_override,
                                             float override_nd, float* out) {
  if (kind == HWY_PE_ROPE) {
    float rx = vals[0] - ex0, ry = vals[1] - ex1;
    float nd = have_override ? override_nd
                             : hm_clipf(__builtin_sqrtf(rx * rx + ry * ry) / max_dist, 0.0f, 1.0f);
#pragma unroll
    for (int f = 0; f < HWY_MAX_FEATURES; ++f)
      if (f < F) {
        if (f < (d & ~1)) {
          const int p = f >> 1;
          float th = (HM_TWO_PI_F * nd) * table[p];
          float s = hm_sinf(th), c = hm_cosf(th);
          float xx = vals[2 * p], yy = vals[2 * p + 1];
          out[f] = (f & 1) ? (xx * s + yy * c) : (xx * c - yy * s);
        } else {
          out[f] = vals[f];
        }
      }
    return;
  }
#pragma unroll
  for (int f = 0; f < HWY_MAX_FEATURES; ++f)
    if (f < F) out[f] = vals[f];
  if (kind == HWY_PE_RANK) {
    for (int k = 0; k < d; ++k) out[F + k] = table[row * d + k];
  } else if (kind == HWY_PE_DIST || kind == HWY_PE_DIST1) {
    float rx = vals[0] - ex0, ry = vals[1] - ex1;
    float dist = kind == HWY_PE_DIST ? __builtin_sqrtf(rx * rx + ry * ry) : hm_absf(rx);
    float nd = have_override ? override_nd : hm_clipf(dist / max_dist, 0.0f, 1.0f);
    const int hd = d / 2;
    for (int k = 0; k < hd; ++k) {
      float ang = (HM_TWO_PI_F * nd) * table[k];
      out[F + k] = hm_sinf(ang);
      out[F + hd + k] = hm_cosf(ang);
    }
  }
}

// KinematicObservation.observe + fused wrapper for the env of this wave.
// ch / sh: hm_cosf / hm_sinf of v.h (the step carries them from the last frame)
// lds_key: WAVE 64-bit words of per-wave LDS scratch (the distance ranking)
// MAP (the observe unit's kernel only, below): *row_map receives the vehicle shown in row `lane`
// (0 for the ego's row, -1 for an empty row and for lanes past the N rows) and a NULL obs_env
// skips the row's store; everything inside `if constexpr (MAP)` is absent from every other caller.
template <bool MAP = false>
__device__ void observe_wave(const hwy_config& C, int lane, const Veh& v, float ch, float sh,
                             int step, uint64_t seed, const float* pe_table, float* obs_env,
                             int fout, int* lds_vor, int* lds_inv, unsigned long long* lds_key,
                             [[maybe_unused]] int* row_map = nullptr) {
  const int V = C.vehicles_count + 1;
  const int N = C.obs_vehicles, F = C.n_features;
  const float ex = rdlf(v.x, 0), ey = rdlf(v.y, 0), eh = rdlf(v.h, 0), espd = rdlf(v.spd, 0);
  const float ec = rdlf(ch, 0), es = rdlf(sh, 0);
  // Road.close_objects_to(ego, PERCEPTION_DISTANCE, count=N-1, see_behind, sort)
  float dx = v.x - ex, dy = v.y - ey;
  bool elig = v.present && lane >= 1 && lane < V &&
              (__builtin_sqrtf(hm_fma(dx, dx, dy * dy)) < PERCEPTION_DISTANCE) &&
              (C.see_behind || -2.0f * VEH_LENGTH < v.x - ex);
  const uint64_t em = ballot(elig);
  int rank;
  if (C.order == HWY_ORDER_SORTED && (kSkip & 64)) {
    rank = __popcll(em & ((1ull << lane) - 1ull));
  } else if (C.order == HWY_ORDER_SORTED) {
    // rank = #{eligible k : |dx_k| < |dx| or (|dx_k| == |dx| and k < lane)}: the bits of |dx|
    // (non-negative: their order is the value order) above the vehicle index make one 64-bit
    // key per vehicle, so a single compare orders by distance and breaks ties by index; an
    // ineligible vehicle holds ~0 and is never below an eligible one.  The keys go through LDS
    // and every lane reads them at the same address (broadcast): two VALU per vehicle
    const unsigned long long ck =
        elig ? ((unsigned long long)hm_f2bits(hm_absf(v.x - ex)) << 32) | (uint32_t)lane : ~0ull;
    lds_key[lane] = ck;
    wave_lds_sync();
    rank = 0;
    for (int k0 = 0; k0 < V; k0 += 2) {
      const unsigned long long k_a = lds_key[k0], k_b = lds_key[k0 + 1];
      rank += k_a < ck ? 1 : 0;
      rank += k_b < ck ? 1 : 0;  // lane k0 + 1 >= V is not present: ~0
    }
    wave_lds_sync();
  } else {
    rank = __popcll(em & ((1ull << lane) - 1ull));
  }
  int nvis = __popcll(em);
  if (nvis > N - 1) nvis = N - 1;
  if (elig && rank < N - 1) lds_vor[rank] = lane;
  // np_random.shuffle(obs[1:]) -> Philox keyed permutation of the N-1 rows
  const bool shuffle = C.order == HWY_ORDER_SHUFFLED && N > 2;
  if (shuffle) {
    uint32_t key = 0u;
    if (lane < N - 1)
      key = hm_philox4x32_10((uint32_t)lane, (uint32_t)step, 0u, 0x53485546u,
                             (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32))
                .v[0];
    int dest = 0;
    for (int p0 = 0; p0 < N - 1; p0 += 4) {
      uint32_t kp[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) kp[u] = (uint32_t)rdli((int)key, min(p0 + u, WAVE - 1));
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = p0 + u;
        dest += (p < N - 1 && (kp[u] < key || (kp[u] == key && p < lane))) ? 1 : 0;
      }
    }
    if (lane < N - 1) lds_inv[dest] = lane;
  }
  wave_lds_sync();
  // output row r = lane
  int kind = 0;  // 0 zero row, 1 ego, 2 other
  int src = 0;
  if (lane == 0) {
    kind = 1;
  } else if (lane < N) {
    int q = shuffle ? lds_inv[lane - 1] : lane - 1;
    if (q < nvis) {
      kind = 2;
      src = lds_vor[q];
    }
  }
  wave_lds_sync();
  const float sx = shf(v.x, src), sy = shf(v.y, src), sspd = shf(v.spd, src), shh = shf(v.h, src);
  const float sc = shf(ch, src), ss = shf(sh, src);
  float vals[HWY_MAX_FEATURES];
#pragma unroll
  for (int f = 0; f < HWY_MAX_FEATURES; ++f) {
    float val = 0.0f;
    if (f < F && kind != 0) {
      int fid = C.feature_ids[f];
      val = feature_value(fid, sx, sy, sspd, shh, sc, ss);
      if (kind == 2 && !C.absolute && is_relative_feature(fid))
        val = val - feature_value(fid, ex, ey, espd, eh, ec, es);
      if (C.normalize && C.has_range[f]) {
        val = hm_lmap(val, C.features_range[f][0], C.features_range[f][1], -1.0f, 1.0f);
        if (C.clip) val = hm_clipf(val, -1.0f, 1.0f);
      }
    }
    vals[f] = val;
  }
  const int eg = C.ego_idx;
  const float ex0 = rdlf(vals[0], eg), ex1 = rdlf(vals[1], eg);
  if constexpr (MAP) {
    *row_map = kind == 0 ? -1 : src;  // kind 1 (the ego's row) holds src = 0
    if (!obs_env) return;             // wave-uniform
  }
  if (lane < N)
    write_pe_row(vals, F, C.pe_kind, C.d_embed, lane, ex0, ex1, C.pe_max_dist, pe_table, false,
                 0.0f, obs_env + (size_t)lane * fout);
}

// ------------------------------------------------------------------------- state I/O

__device__ __forceinline__ void load_veh(const uint32_t* st, size_t fstride, uint32_t idx, int lane,
                                         int V, Veh& v, int& order_pos) {
  v.x = hm_bits2f((st + HWY_F_X * fstride)[idx]);
  v.y = hm_bits2f((st + HWY_F_Y * fstride)[idx]);
  v.h = hm_bits2f((st + HWY_F_HEADING * fstride)[idx]);
  v.spd = hm_bits2f((st + HWY_F_SPEED * fstride)[idx]);
  v.tsp = hm_bits2f((st + HWY_F_TSPEED * fstride)[idx]);
  v.dlt = hm_bits2f((st + HWY_F_DELTA * fstride)[idx]);
  v.tmr = hm_bits2f((st + HWY_F_TIMER * fstride)[idx]);
  v.ix = hm_bits2f((st + HWY_F_IMPX * fstride)[idx]);
  v.iy = hm_bits2f((st + HWY_F_IMPY * fstride)[idx]);
  v.ln = (int)(st + HWY_F_LANE * fstride)[idx];
  v.tl = (int)(st + HWY_F_TLANE * fstride)[idx];
  uint32_t fl = (st + HWY_F_FLAGS * fstride)[idx];
  v.crashed = (fl & HWY_FLAG_CRASHED) != 0u;
  v.imp = (fl & HWY_FLAG_IMPACT) != 0u;
  v.present = ((fl & HWY_FLAG_PRESENT) != 0u) && lane < V;
  order_pos = (int)((fl & HWY_FLAG_ORDER_MASK) >> HWY_FLAG_ORDER_SHIFT);
  v.aacc = 0.0f;
  v.asteer = 0.0f;
}

__device__ __forceinline__ void store_veh(uint32_t* st, size_t fstride, uint32_t idx, int lane, int V,
                                          const Veh& v, int order_pos) {
  // opaque copies of the offset, the base and the field stride: the 13 field addresses are
  // rebuilt here instead of being kept live from load_veh across the whole step (26 VGPRs for the
  // lane addresses, 26 SGPRs for the field bases, which otherwise spill the frame loop's scalars)
  asm volatile("" : "+v"(idx));
  asm volatile("" : "+s"(st));
  asm volatile("" : "+s"(fstride));
  const bool live = lane < V;
  (st + HWY_F_X * fstride)[idx] = live ? hm_f2bits(v.x) : 0u;
  (st + HWY_F_Y * fstride)[idx] = live ? hm_f2bits(v.y) : 0u;
  (st + HWY_F_HEADING * fstride)[idx] = live ? hm_f2bits(v.h) : 0u;
  (st + HWY_F_SPEED * fstride)[idx] = live ? hm_f2bits(v.spd) : 0u;
  (st + HWY_F_TSPEED * fstride)[idx] = live ? hm_f2bits(v.tsp) : 0u;
  (st + HWY_F_DELTA * fstride)[idx] = live ? hm_f2bits(v.dlt) : 0u;
  (st + HWY_F_TIMER * fstride)[idx] = live ? hm_f2bits(v.tmr) : 0u;
  (st + HWY_F_IMPX * fstride)[idx] = (live && v.imp) ? hm_f2bits(v.ix) : 0u;
  (st + HWY_F_IMPY * fstride)[idx] = (live && v.imp) ? hm_f2bits(v.iy) : 0u;
  (st + HWY_F_LANE * fstride)[idx] = live ? (uint32_t)v.ln : 0u;
  (st + HWY_F_TLANE * fstride)[idx] = live ? (uint32_t)v.tl : 0u;
  (st + HWY_F_FLAGS * fstride)[idx] =
      live ? ((v.crashed ? HWY_FLAG_CRASHED : 0u) | (v.imp ? HWY_FLAG_IMPACT : 0u) |
              (v.present ? HWY_FLAG_PRESENT : 0u) |
              ((uint32_t)order_pos << HWY_FLAG_ORDER_SHIFT))
           : 0u;
}

__device__ __forceinline__ void store_env_words(uint32_t* st, size_t fstride, uint32_t idx, int lane,
                                                int step, int episode, uint64_t seed, float ego_acc,
                                                float ego_steer, float ep_return) {
  asm volatile("" : "+v"(idx));
  asm volatile("" : "+s"(st));
  asm volatile("" : "+s"(fstride));
  uint32_t w = 0u;
  if (lane == HWY_E_STEP) w = (uint32_t)step;
  if (lane == HWY_E_EPISODE) w = (uint32_t)episode;
  if (lane == HWY_E_SEED_LO) w = (uint32_t)(seed & 0xffffffffu);
  if (lane == HWY_E_SEED_HI) w = (uint32_t)(seed >> 32);
  if (lane == HWY_E_EGO_ACC) w = hm_f2bits(ego_acc);
  if (lane == HWY_E_EGO_STEER) w = hm_f2bits(ego_steer);
  if (lane == HWY_E_RETURN) w = hm_f2bits(ep_return);
  (st + HWY_F_ENV * fstride)[idx] = w;
}

// ------------------------------------------------------------------------- road order
// The vehicles of a wave sorted by (x ascending, index descending), kept across the frames of
// a step: lane p of `ord` holds the vehicle at position p, `rk` is this lane's position.
// Absent lanes sort after every present vehicle, so the positions form a permutation of 0..63.
struct RoadOrder {
  int rk, ord;
  bool valid;
};

__device__ __forceinline__ uint64_t shf64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)shi((int)(uint32_t)v, src);
  const uint32_t hi = (uint32_t)shi((int)(uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t shl1_64(uint64_t v) {
  return ((uint64_t)(uint32_t)shl1i((int)(uint32_t)(v >> 32)) << 32) |
         (uint32_t)shl1i((int)(uint32_t)v);
}
__device__ __forceinline__ uint64_t shr1_64(uint64_t v) {
  return ((uint64_t)(uint32_t)shr1i((int)(uint32_t)(v >> 32)) << 32) |
         (uint32_t)shr1i((int)(uint32_t)v);
}
__device__ __forceinline__ uint64_t swp1_64(uint64_t v) {
  return ((uint64_t)(uint32_t)swp1i((int)(uint32_t)(v >> 32)) << 32) |
         (uint32_t)swp1i((int)(uint32_t)v);
}

// order-preserving u32 image of x (+0 and -0 map together); absent -> above every float
__device__ __forceinline__ uint64_t road_key(float x, bool present, int lane) {
  const uint32_t u = hm_f2bits(x + 0.0f);
  uint32_t s = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  if (!present) s = 0xffffffffu;
  return ((uint64_t)s << 32) | (uint32_t)(WAVE - 1 - lane);
}

// Re-validates (or rebuilds) the order for the current positions.
__device__ void road_order(int lane, const Veh& v, uint64_t pres, RoadOrder& o) {
  const uint64_t key = road_key(v.x, v.present, lane);
  bool sorted = false;
  if (o.valid) {
    uint64_t kp = shf64(key, o.ord);
    uint64_t kn = shl1_64(kp);  // the next position's key (DPP)
    sorted = (~ballot(kp < kn) & (~0ull >> 1)) == 0ull;  // every position but the last ascends
    // a few overtakes since the last frame: odd-even transposition rounds on (key, vehicle)
    // in position space usually restore the order without a full re-rank; the partner is
    // lane ^ 1 in the even phase and lane + 1 / lane - 1 (odd / even lane) in the odd one
    int ordp = o.ord;
    for (int round = 0; round < 3 && !sorted; ++round) {
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        const bool left = (lane & 1) == ph;
        int partner = left ? lane + 1 : lane - 1;
        if (partner < 0 || partner >= WAVE) partner = lane;
        uint64_t pk;
        int po;
        if (ph == 0) {
          pk = swp1_64(kp);
          po = swp1i(ordp);
        } else {
          const uint64_t up = shl1_64(kp), dn = shr1_64(kp);
          const int uo = shl1i(ordp), dno = shr1i(ordp);
          pk = left ? up : dn;
          po = left ? uo : dno;
        }
        const bool swap = partner != lane && (left ? (pk < kp) : (kp < pk));
        kp = swap ? pk : kp;
        ordp = swap ? po : ordp;
      }
      kn = shl1_64(kp);
      sorted = (~ballot(kp < kn) & (~0ull >> 1)) == 0ull;
    }
    if (sorted) {
      o.ord = ordp;
      o.rk = __builtin_amdgcn_ds_permute(ordp << 2, lane);  // vehicle ordp sits at position lane
    }
  }
  if (!sorted) {
    int r = 0;
    if (v.present) {
      for (int k = 0; k < WAVE; ++k) {
        if (!((pres >> k) & 1ull)) continue;
        const uint64_t kk = ((uint64_t)(uint32_t)rdli((int)(key >> 32), k) << 32) |
                            (uint32_t)(WAVE - 1 - k);
        r += kk < key ? 1 : 0;
      }
    } else {  // absent lanes: after all present ones, by descending lane index
      const uint64_t above = lane >= WAVE - 1 ? 0ull : (~0ull << (lane + 1));
      r = __popcll(pres) + __popcll(~pres & above);
    }
    o.rk = r;
    o.ord = __builtin_amdgcn_ds_permute(r << 2, lane);
    o.valid = true;
  }
}

// Road.neighbour_vehicles(self, lane c) for c = ln-1, ln, ln+1 (slot s <-> c = ln-1+s) from the
// road order: for each lane c a 64-bit mask over positions of the vehicles with
// on_lane(c, margin 1).  Upstream scans the list in index order with `s <= s_v and s_v <=
// s_front` (front: nearest x ahead or level, the LAST such vehicle on a tie) and `s_v < s and
// s_v > s_rear` (rear: nearest x strictly behind, the FIRST on a tie).  Equal x sit together in
// the order by descending index, so with g = the first position of this vehicle's x group the
// front is the lowest set position >= g other than its own, the rear the highest below g.  NaN
// positions fail on_lane; a vehicle at NaN itself finds nothing (every comparison is false).
struct LaneScan {
  float yp;      // y of the vehicle at position `lane`
  bool okp;      // that vehicle is present and inside the road's x range
  uint64_t okm;  // ballot(okp)
  uint64_t ahead, behind;  // candidate positions for the front / the rear of this vehicle
};

// xp: x of the vehicle at position `lane` (shf(v.x, o.ord), when the caller has it)
__device__ __forceinline__ LaneScan lane_scan(int lane, const Veh& v, uint64_t pres,
                                              const RoadOrder& o, float xp) {
  LaneScan L;
  const int npres = __popcll(pres);
  L.yp = shf(v.y, o.ord);
  L.okp = lane < npres && -LANE_VEH_LEN <= xp && xp < ROAD_LENGTH + LANE_VEH_LEN;
  L.okm = ballot(lane < npres) & ballot(-LANE_VEH_LEN <= xp) & ballot(xp < ROAD_LENGTH + LANE_VEH_LEN);
  const float xprev = shr1f(xp);
  const uint64_t starts = ballot(xprev != xp) | 1ull;  // x-group starts (bit 0 set)
  const int g = 63 - __builtin_clzll(starts & ((2ull << o.rk) - 1ull));  // rk = 63: all ones
  const bool selfok = v.x == v.x;
  L.ahead = selfok ? (~0ull << g) & ~(1ull << o.rk) : 0ull;
  L.behind = selfok ? (1ull << g) - 1ull : 0ull;
  return L;
}

__device__ __forceinline__ uint64_t on_lane_mask(const LaneScan& L, int c) {
  // (the compare's own mask, then a scalar AND: a ballot of p && q costs two VALU more)
  return ballot(hm_absf(lane_lat(L.yp, c)) <= LANE_WIDTH / 2.0f + 1.0f) & L.okm;
}

// Also returns qf[s], the road-order position of front s (this vehicle's own position when
// there is none), for gathers from position-space copies one bpermute level earlier.
__device__ __forceinline__ void neighbours_ordered(const hwy_config& C, int lane, const Veh& v,
                                                   uint64_t pres, const RoadOrder& o, float xq,
                                                   int fi[3], int ri[3], int qfp[3]) {
  const LaneScan L = lane_scan(lane, v, pres, o, xq);
  uint64_t m[3] = {0ull, 0ull, 0ull};
  if (C.lanes_count <= WAVE - 2) {
    // lane c's position mask (wave-uniform) goes to lane c + 1 of a VGPR pair (lanes 0 and
    // lanes_count + 1 .. 63 hold no lane: 0), and each vehicle reads its slots ln .. ln + 2
    int tlo = 0, thi = 0;
    for (int c = 0; c < C.lanes_count; ++c) {
      const uint64_t mc = on_lane_mask(L, c);
      const bool mine = lane == c + 1;
      tlo = mine ? (int)(uint32_t)mc : tlo;
      thi = mine ? (int)(uint32_t)(mc >> 32) : thi;
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int src = v.ln + s;  // slot of lane ln - 1 + s
      const bool in = src >= 0 && src < WAVE;
      const int q = in ? src : 0;
      const uint64_t mq = ((uint64_t)(uint32_t)shi(thi, q) << 32) | (uint32_t)shi(tlo, q);
      m[s] = in ? mq : 0ull;
    }
  } else {
    for (int c = 0; c < C.lanes_count; ++c) {
      const uint64_t mc = on_lane_mask(L, c);
#pragma unroll
      for (int s = 0; s < 3; ++s)
        if (c == v.ln - 1 + s) m[s] = mc;
    }
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const uint64_t fa = m[s] & L.ahead, rb = m[s] & L.behind;
    const int qf = fa ? __builtin_ctzll(fa) : 0;
    const int qr = rb ? 63 - __builtin_clzll(rb) : 0;
    const int vf = shi(o.ord, qf), vr = shi(o.ord, qr);
    fi[s] = fa ? vf : -1;
    ri[s] = rb ? vr : -1;
    qfp[s] = fa ? qf : o.rk;
  }
}

// the front vehicle on an arbitrary lane c of each vehicle (same rule as neighbours_ordered)
__device__ __forceinline__ int front_on_lane(const hwy_config& C, int lane, const Veh& v,
                                             uint64_t pres, const RoadOrder& o, int c_own) {
  const LaneScan L = lane_scan(lane, v, pres, o, shf(v.x, o.ord));
  uint64_t m = 0ull;
  for (int c = 0; c < C.lanes_count; ++c) {
    const uint64_t mc = on_lane_mask(L, c);
    if (c == c_own) m = mc;
  }
  const uint64_t fa = m & L.ahead;
  const int vf = shi(o.ord, fa ? __builtin_ctzll(fa) : 0);
  return fa ? vf : -1;
}

// per-wave LDS of the collision pass (5.4 KB)
struct CollLds {
  unsigned long long imx[WAVE], imy[WAVE];  // (partner + 1) << 32 | impact bits, max-reduced
  int crash[WAVE];
  int pord[WAVE];                         // vehicle at each road-order position
  uint16_t plist[WAVE * (WAVE - 1) / 2];  // candidate pairs (a << 8 | b), a < b
};

// ------------------------------------------------------------------------- one frame
// Road.act() then Road.step(dt) for the env of this wave (lane = vehicle).
// pres: ballot(v.present), fixed for the step (presence changes only at a reset)
__device__ void frame_wave(const hwy_config& C, int lane, Veh& v, float dt, float tan_ego, RoadOrder& ro,
                           float& cos_h, float& sin_h, CollLds& cl, SecProf& sp, uint64_t pres) {
  const int lanes = C.lanes_count;
  const float limit = C.speed_limit;
  const float ch = cos_h, sh = sin_h;  // cos / sin of v.h (carried from the previous frame)

  // ---------------- Road.act: IDMVehicle.act for every non-crashed traffic car
  const bool actor = v.present && lane >= 1 && !v.crashed;
  const int tl_old = v.tl;
  const bool mid = v.ln != v.tl;
  const bool fire = actor && !mid && (LANE_CHANGE_DELAY < v.tmr);  // utils.do_every
  // (wave masks from the compares' own masks: a ballot of a compound bool costs two VALU)
  const uint64_t actm = pres & ~1ull & ~ballot(v.crashed);  // ballot(actor)
  const uint64_t firem = actm & ~ballot(v.ln != v.tl) & ballot(LANE_CHANGE_DELAY < v.tmr);
  if (fire) v.tmr = 0.0f;

  // Road.neighbour_vehicles on lanes ln-1, ln, ln+1 (slot s <-> lane ln-1+s)
  int fi[3], ri[3];
  SEC(sp, 0);
  if (!ro.valid) road_order(lane, v, pres, ro);  // later frames: validated after the last move
  SEC(sp, 9);
  // position-space copies of the fronts' state (vehicle at position p on lane p), gathered
  // alongside the order so the fronts' values are one bpermute from their positions
  // this vehicle's velocity vector (Vehicle.velocity), shared by every desired_gap of the frame
  const float vvx = v.spd * ch, vvy = v.spd * sh;
  const float xq = shf(v.x, ro.ord), vxq = shf(vvx, ro.ord), vyq = shf(vvy, ro.ord);
  int qfp[3];
  neighbours_ordered(C, lane, v, pres, ro, xq, fi, ri, qfp);
  SEC(sp, 1);

  // gathers (all lanes active); a missing front reads this vehicle's own values (unused)
  const int sop = qfp[1];
  const float op_x = shf(xq, sop), op_vx = shf(vxq, sop), op_vy = shf(vyq, sop);
  float np_x[2], np_vx[2], np_vy[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int a = qfp[2 * q];  // slot 0 (left, ln-1) and slot 2 (right, ln+1)
    np_x[q] = shf(xq, a);
    np_vx[q] = shf(vxq, a);
    np_vy[q] = shf(vyq, a);
  }

  // acceleration(self, front on own lane): IDM term and MOBIL's self_a
  float self_a = 0.0f;
  // (the free-road term is shared by every acceleration(self, .) evaluated this frame)
  // every lane's free-road base and its log (the ego as a plain Vehicle: target speed 0), also
  // read by mobil for a new follower (same base, the deciding vehicle's DELTA)
  const float fbase = idm_base(v.spd, lane == 0 ? 0.0f : v.tsp, limit);
  const float flog = hm_logf_idm(fbase);
  float a_free = 0.0f;
  if (actor) {
    a_free = idm_free_from(fbase, flog, v.dlt);
    self_a = idm_with_front(a_free, v.spd, v.x, ch, sh, vvx, vvy, fi[1] >= 0, op_x, op_vx, op_vy);
  }

  // IDMVehicle.change_lane_policy -> mobil, side lanes left then right (POLITENESS = 0, so the
  // followers' unchanged-lane terms multiply by zero and are not evaluated).  mobil's two tests
  // are pure and both must hold, so the cheap one (own acceleration gain, free-road term shared)
  // runs first, and the new followers' data and IDM (a pow) only for the candidates that would
  // gain -- rarely any in a frame; the decision is upstream's.
  SEC(sp, 2);
  int ntl = v.tl;
  // (every lane evaluates both sides when any lane fires -- a lane without a front on a side,
  // or outside the lanes, reads a_free -- and the lane's own tests mask the result)
  bool gain[2] = {false, false};
  uint64_t gainm = 0ull;
  // the side-independent tests, once (a ballot of a compare used again under another branch
  // re-materialises too)
  const uint64_t basem = firem & ballot(0.0f <= v.x) & ballot(v.x < ROAD_LENGTH + LANE_VEH_LEN) &
                         ~ballot(hm_absf(v.spd) < 1.0f);
  if (basem && !(kSkip & 1)) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = v.ln - 1 + 2 * q;
      const int s = 2 * q;
      const float spa = idm_with_front(a_free, v.spd, v.x, ch, sh, vvx, vvy, fi[s] >= 0, np_x[q],
                                       np_vx[q], np_vy[q]);
      const bool in_lanes = c >= 0 && c < lanes;
      const bool reach = hm_absf(lane_lat(v.y, c)) <= 2.0f * LANE_WIDTH && 0.0f <= v.x &&
                         v.x < ROAD_LENGTH + LANE_VEH_LEN;  // is_reachable_from
      const bool slow = hm_absf(v.spd) < 1.0f;
      const bool loss = (spa - self_a) < LANE_CHANGE_MIN_ACC_GAIN;
      gain[q] = fire && in_lanes && reach && !slow && !loss;
      gainm |= basem & ballot(c >= 0) & ballot(c < lanes) &
               ballot(hm_absf(lane_lat(v.y, c)) <= 2.0f * LANE_WIDTH) & ~ballot(loss);
    }
  }
  if (gainm) {
    // upstream tries left, then right, and a passing right side overrides the left: so each
    // lane first evaluates the side that decides if it passes -- the right where it gains, else
    // the left -- in one pass over the lanes (one new-follower IDM, a pow, instead of two), and
    // only lanes whose right side gained but failed the braking test evaluate their left side
    // after it (rare).  The same arithmetic per side as the sequential order, so the same bits.
    auto new_follower_ok = [&](int q) {
      const int rq = q ? ri[2] : ri[0];
      const int b = rq >= 0 ? rq : lane;  // all lanes active: ds_bpermute
      const float nf_x = shf(v.x, b), nf_spd = shf(v.spd, b), nf_c = shf(ch, b), nf_s = shf(sh, b);
      const float nf_base = shf(fbase, b), nf_log = shf(flog, b);
      float nfp = 0.0f;
      if (rq >= 0)  // acceleration(ego_vehicle=new follower, front_vehicle=self), self's DELTA
        nfp = idm_with_front(idm_free_from(nf_base, nf_log, v.dlt), nf_spd, nf_x, nf_c, nf_s,
                             nf_spd * nf_c, nf_spd * nf_s, true, v.x, vvx, vvy);
      return !(nfp < -LANE_CHANGE_MAX_BRAKING_IMPOSED);
    };
    const int q1 = gain[1] ? 1 : 0;
    const bool nok = new_follower_ok(q1);  // every lane (the gathers need all 64 active)
    const bool ok1 = (gain[0] || gain[1]) && nok;
    if (ok1) ntl = v.ln - 1 + 2 * q1;
    const bool retry = gain[1] && !ok1 && gain[0];
    if (wave_any(retry)) {
      const bool ok0 = new_follower_ok(0);
      if (retry && ok0) ntl = v.ln - 1;
    }
  }

  SEC(sp, 3);
  // abort an ongoing lane change if another car targets the same lane within its desired gap,
  // in road order (lower indices already final, higher ones at their frame-start target)
  int tl_cur = ntl;
  uint64_t cm = (kSkip & 8) ? 0ull : actm & ballot(v.ln != v.tl);  // actor && mid
  // a lane can trigger an abort only while its visible target is not its own lane (vis == tj
  // and ln != tj), under either visibility; aborts only ever clear that, so this superset holds
  // for the whole loop
  const uint64_t canm = pres & ~1ull & (ballot(tl_cur != v.ln) | ballot(tl_old != v.ln));
  while (cm) {
    const int j = __builtin_ctzll(cm);
    cm &= cm - 1ull;
    const int tj = rdli(tl_cur, j);
    const int vis = (lane < j) ? tl_cur : tl_old;
    // the target-lane part of upstream's test first: most vehicles find no other car targeting
    // their lane, and then the gap test (four broadcasts and a desired_gap) is skipped
    const uint64_t cheapm = canm & ~(1ull << j) & ballot(v.ln != tj) & ballot(vis == tj);
    if (!cheapm) continue;
    const float xj = rdlf(v.x, j), vj = rdlf(v.spd, j), cj = rdlf(ch, j), sj = rdlf(sh, j);
    const float d = v.x - xj;
    const float d_star = desired_gap_v(vj, cj, sj, vj * cj, vj * sj, vvx, vvy);
    const uint64_t condm = cheapm & ballot(0.0f < d) & ballot(d < d_star);
    if (condm && lane == j) tl_cur = v.ln;
  }
  v.tl = tl_cur;

  SEC(sp, 4);
  // IDM on the target lane while changing lanes
  const bool need_t = actor && v.ln != v.tl;
  int ft = -1;
  if (v.tl == v.ln - 1) ft = fi[0];
  if (v.tl == v.ln + 1) ft = fi[2];
  const bool extra = need_t && !(v.tl == v.ln - 1 || v.tl == v.ln + 1);
  if (actm & ballot(v.ln != v.tl) & ~ballot(v.tl == v.ln - 1) & ~ballot(v.tl == v.ln + 1)) {  // target lane not adjacent (rare): its own lane mask
    const int fx = front_on_lane(C, lane, v, pres, ro, v.tl);
    if (extra) ft = fx;
  }
  const int st_ = ft >= 0 ? ft : lane;
  const float ft_x = shf(v.x, st_), ft_vx = shf(vvx, st_), ft_vy = shf(vvy, st_);
  if (actor) {
    const float steer = (kSkip & 16) ? 0.0f : steering_tan(v.y, v.h, v.spd, v.tl);
    float acc = self_a;
    if (need_t) {
      const float acc_t =
          idm_with_front(a_free, v.spd, v.x, ch, sh, vvx, vvy, ft >= 0, ft_x, ft_vx, ft_vy);
      acc = hm_minf(acc, acc_t);
    }
    acc = hm_clipf(acc, -ACC_MAX, ACC_MAX);
    v.asteer = steer;
    v.aacc = acc;
  }

  SEC(sp, 5);
  // ---------------- Road.step: Vehicle.step for every vehicle
  if (v.present) {
    if (lane != 0) v.tmr = v.tmr + dt;  // IDMVehicle.step
    if (v.crashed) {                    // clip_actions
      v.asteer = 0.0f;
      v.aacc = -1.0f * v.spd;
    }
    if (v.spd > MAX_SPEED) {
      v.aacc = hm_minf(v.aacc, 1.0f * (MAX_SPEED - v.spd));
    } else if (v.spd < MIN_SPEED) {
      v.aacc = hm_maxf(v.aacc, 1.0f * (MIN_SPEED - v.spd));
    }
    // beta = atan(tan(steering) / 2) in closed form (oracle vehicle_step): cos and sin of beta
    // from u = tan(beta), cos / sin of h + beta by angle addition from the carried cos / sin h
    const float u = 0.5f * ((lane == 0 && !v.crashed) ? tan_ego : v.asteer);
    const float cb = 1.0f / __builtin_sqrtf(hm_fma(u, u, 1.0f));
    const float sb = u * cb;
    const float cdir = hm_fma(ch, cb, -(sh * sb));
    const float sdir = hm_fma(sh, cb, ch * sb);
    const float vx = v.spd * cdir;
    const float vy = v.spd * sdir;
    v.x = hm_fma(vx, dt, v.x);
    v.y = hm_fma(vy, dt, v.y);
    if (v.imp) {
      v.x = v.x + v.ix;
      v.y = v.y + v.iy;
      v.crashed = true;
      v.imp = false;
    }
    v.h = hm_fma(v.spd * sb, dt * (2.0f / VEH_LENGTH), v.h);  // speed sin(beta) / (L/2) dt
    v.spd = hm_fma(v.aacc, dt, v.spd);
    v.ln = closest_lane(v.y, lanes);  // on_state_update
  }

  SEC(sp, 6);
  // ---------------- Road.step: handle_collisions for every pair, a = lower index
  float c2, s2;
  hm_sincosf(v.h, &s2, &c2);
  cos_h = c2;
  sin_h = s2;
  road_order(lane, v, pres, ro);  // new positions; also serves the next frame's neighbours
  SEC(sp, 7);
  // Candidates first: a pair can pass the centre-distance pre-check only if |dx| is within
  // that bound, taken here with the wave's largest speed (and widened past any rounding; a
  // non-finite speed or position disables the filter).
  float vabs = v.present ? hm_absf(v.spd) : 0.0f;
  // any present vehicle with a non-finite x, y or speed (the compares' own masks)
  const uint64_t nonfinite = pres & (ballot(!(hm_absf(v.x) <= 3.0e38f)) |
                                     ballot(!(hm_absf(v.y) <= 3.0e38f)) |
                                     ballot(!(hm_absf(v.spd) <= 3.0e38f)));
  vabs = wave_max_f(vabs);
  const float xbound = nonfinite ? __builtin_huge_valf()
                                 : (VEH_DIAGONAL + vabs * dt) * 1.001f + 1.0e-3f;
  // x-sorted road order, in position space (lane = position p, holding vehicle ord[p]): the
  // candidates are the pairs (p, p+o) whose |dx| is within the bound.  x is monotone along the
  // order, so the run from p upwards is contiguous and every pair is found once, from its lower
  // position; x at p+o comes from a one-lane DPP shift per step (equal x sit together; a NaN x,
  // or any non-finite value, makes the bound infinite: every pair of present vehicles).
  int run = 0;  // the candidates of position p: (p, p + o) for o = 1 .. run
  {
    const int npres = __popcll(pres);
    const float xs = shf(v.x, ro.ord);  // x at position `lane`
    float xu = xs;
    // the loop runs on the wave mask U = ballot(up), kept from the compares' own masks (a
    // ballot of a compound or loop-carried bool re-materialises it: two VALU), and counts each
    // position's run; its candidates are o = 1 .. run
    bool up = lane < npres;
    uint64_t U = (kSkip & 4) ? 0ull : ballot(lane < npres);
    for (int o = 1; U; ++o) {
      xu = __int_as_float(shl1i(__float_as_int(xu)));  // x at position lane + o
      const bool inr = lane < npres - o;
      const bool far = hm_absf(xu - xs) > xbound;
      up = up && inr && !far;
      U &= ballot(inr) & ~ballot(far);
      run += up ? 1 : 0;
    }
  }
  SEC(sp, 10);
  // Each candidate pair once, spread over the lanes: position p lists its pairs (as vehicle
  // indices a < b) at its exclusive prefix offset, then lane t takes pair t (64 per round).
  // Per vehicle, upstream keeps the impact of its highest-index partner (the last
  // handle_collisions call that writes it) and ORs the crash flag; the translation therefore
  // goes through a 64-bit LDS max keyed by (partner + 1) in the high word.
  const int cnt = run;
  int off = wave_incl_scan(cnt);
  const int total = rdli(off, WAVE - 1);
  off -= cnt;
  cl.imx[lane] = 0ull;
  cl.imy[lane] = 0ull;
  cl.crash[lane] = 0;
  cl.pord[lane] = ro.ord;
  wave_lds_sync();
  // (a loop over o = 1 .. run measured the same time with more VALU, round 5)
  uint64_t om = (2ull << run) - 2ull;  // bits 1 .. run (run <= 63)
  while (om) {
    const int o = __builtin_ctzll(om);
    om &= om - 1ull;
    const int q = cl.pord[lane + o];
    const int lo = ro.ord < q ? ro.ord : q, hi = ro.ord < q ? q : ro.ord;
    cl.plist[off++] = (uint16_t)((lo << 8) | hi);
  }
  wave_lds_sync();
  for (int base = 0; base < ((kSkip & 2) ? 0 : total); base += WAVE) {
    const bool has = base + lane < total;
    const int pr = has ? cl.plist[base + lane] : 0;
    const int a = pr >> 8, b = pr & 0xff;  // a < b
    const float xa = shf(v.x, a), ya = shf(v.y, a), ca = shf(c2, a), sa = shf(s2, a),
                va = shf(v.spd, a);
    const float xb = shf(v.x, b), yb = shf(v.y, b), cb = shf(c2, b), sb = shf(s2, b),
                vb = shf(v.spd, b);
    // exact pre-check (are_polygons_intersecting is only called inside it), then the SAT test
    const float dx = xb - xa, dy = yb - ya;
    // upstream's sqrt(dx^2 + dy^2) > B, decided from the squares where they are 2^-19 apart (a
    // margin far above the roundings of B^2 and of the thresholds: the correctly rounded root
    // lies on the same side of B); a lane near the boundary, with B outside [1e-10, 2^60) or a
    // non-finite square, takes the root itself
    const float q2 = hm_fma(dx, dx, dy * dy);
    const float bb = (VEH_DIAGONAL + VEH_DIAGONAL) / 2.0f + va * dt;
    const float b2 = bb * bb;
    const uint64_t bokm = ballot(bb >= 1.0e-10f) & ballot(bb < 0x1p60f);
    const bool gt = q2 > b2 * (1.0f + 0x1p-19f), lt = q2 < b2 * (1.0f - 0x1p-19f);
    bool far = gt;
    uint64_t farm = ballot(gt);  // ballot(far), from the compare's own mask on the usual path
    if (~(bokm & (farm | ballot(lt)))) {  // some lane undecided (rare): its root
      const bool sure = (bb >= 1.0e-10f && bb < 0x1p60f) && (gt || lt);
      far = sure ? gt : __builtin_sqrtf(q2) > bb;
      farm = ballot(far);
    }
    bool pass = has && !far;
    uint64_t passm = ballot(lane < total - base) & ~farm;  // ballot(pass)
    if (!passm) continue;
    const float dax = (va * ca) * dt, day = (va * sa) * dt, dbx = (vb * cb) * dt, dby = (vb * sb) * dt;
    // a's v axis (the SAT's second edge normal) first: a pair separated on it both as it stands
    // and swept by the velocities ends with intersecting = will_intersect = false and no
    // translation whatever the other axes give (the SAT only ever clears the two flags), so it
    // leaves the round; rounds whose pairs all leave skip the SAT (cars side by side in adjacent
    // lanes).  The same operations as sat_collide's edge 1, so the decision is exact.
    {
      float a0, a1, b0, b1;
      rect_interval(xa, ya, ca, sa, -sa, ca, a0, a1);
      rect_interval(xb, yb, cb, sb, -sa, ca, b0, b1);
      const float vp = hm_fma(-sa, dax - dbx, ca * (day - dby));
      const bool sep0 = interval_distance(a0, a1, b0, b1) > 0.0f;
      const bool sep1 = interval_distance(vp < 0.0f ? a0 + vp : a0, vp < 0.0f ? a1 : a1 + vp, b0,
                                          b1) > 0.0f;
      pass = pass && !(sep0 && sep1);
      passm &= ~(ballot(sep0) & ballot(sep1));
      if (!passm) continue;
    }
    bool inter, will;
    float tx, ty;
    sat_collide(passm, xa, ya, ca, sa, dax, day, xb, yb, cb, sb, dbx, dby, &inter, &will, &tx, &ty);
    if (pass && will) {
      atomicMax(&cl.imx[a], ((uint64_t)(b + 1) << 32) | hm_f2bits(tx / 2.0f));
      atomicMax(&cl.imy[a], ((uint64_t)(b + 1) << 32) | hm_f2bits(ty / 2.0f));
      atomicMax(&cl.imx[b], ((uint64_t)(a + 1) << 32) | hm_f2bits(-tx / 2.0f));
      atomicMax(&cl.imy[b], ((uint64_t)(a + 1) << 32) | hm_f2bits(-ty / 2.0f));
    }
    if (pass && inter) {
      cl.crash[a] = 1;
      cl.crash[b] = 1;
    }
  }
  wave_lds_sync();
  const uint64_t mx = cl.imx[lane], my = cl.imy[lane];
  if (mx != 0ull) {
    v.ix = hm_bits2f((uint32_t)mx);
    v.iy = hm_bits2f((uint32_t)my);
    v.imp = true;
  }
  if (cl.crash[lane]) v.crashed = true;
  wave_lds_sync();  // the lists are rewritten next frame
  SEC(sp, 8);
}

// ------------------------------------------------------------------------- kernels
// W: waves per SIMD the registers are sized for.  4 (106 VGPRs) when the envs fit one wave per
// env on 4 waves per SIMD (4,096 envs on 256 CUs: 0.160 ms); 6 (80 VGPRs, 14 spilled to scratch
// outside the hot loop) when more envs queue behind them: 16,384 envs 0.412 -> 0.365 ms,
// 32,768 0.775 -> 0.670 (5 waves: 0.381 / 0.702), 8,192 0.228 -> 0.220; at 4,096 envs the 6-wave
// build takes 0.164 ms, so hwy_launch_step picks by env count (round 6, launch parameters from a
// table: the 4-wave build also wins at 8,192 envs, so the 6-wave one starts above 32 envs per CU)
// The step of one handle's envs; the kernels below run it for one handle (hwy_step) or for
// handle blockIdx.y of a table (hwy_step_group: a sweep's cells in one launch).  It reads no
// gridDim and no blockIdx.y, so a grouped launch computes every env exactly as its handle's own.
// INFO (the info unit's kernels only, below): the ego's per-step info and the running episode
// sums go to *I; everything inside `if constexpr (INFO)` is absent from the plain kernels.
// FINAL (the final unit's kernels only): the finished episode's last observation goes to
// final_obs before the autoreset; absent from the plain and the info kernels likewise.
template <int W, bool INFO, bool FINAL = false>
__device__ __forceinline__ void step_body(const StepParams& P, const InfoParams* I,
                                          [[maybe_unused]] float* final_obs = nullptr) {
  __shared__ int lds_vor[ENVS_PER_BLOCK][WAVE];
  __shared__ int lds_inv[ENVS_PER_BLOCK][WAVE];
  __shared__ CollLds lds_coll[ENVS_PER_BLOCK];
  const hwy_config& C = P.cfg;
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = threadIdx.x / WAVE;
  const int e = blockIdx.x * ENVS_PER_BLOCK + w;
  if (e >= C.num_envs) return;  // whole wave
  const int V = C.vehicles_count + 1;
  const size_t fstride = (size_t)C.num_envs * WAVE;
  const uint32_t idx = (uint32_t)e * WAVE + lane;  // < 2^32: hwy_create bounds num_envs
  uint32_t* st = P.state;

  SecProf sp;
  SEC_START(sp);
  WAVE_T(e, lane, 0, __builtin_amdgcn_s_memtime());
  WAVE_T(e, lane, 3, __builtin_amdgcn_s_memrealtime());
  Veh v;
  int order_pos;
  load_veh(st, fstride, idx, lane, V, v, order_pos);
  [[maybe_unused]] const int ln_start = v.ln;  // INFO: the lane word as loaded
  const uint32_t ew = (st + HWY_F_ENV * fstride)[idx];
  int step = rdli((int)ew, HWY_E_STEP);
  int episode = rdli((int)ew, HWY_E_EPISODE);
  uint64_t seed = (uint64_t)(uint32_t)rdli((int)ew, HWY_E_SEED_LO) |
                  ((uint64_t)(uint32_t)rdli((int)ew, HWY_E_SEED_HI) << 32);
  float ep_return = hm_bits2f((uint32_t)rdli((int)ew, HWY_E_RETURN));
  if (lane == 0) {
    v.aacc = hm_bits2f((uint32_t)rdli((int)ew, HWY_E_EGO_ACC));
    v.asteer = hm_bits2f((uint32_t)rdli((int)ew, HWY_E_EGO_STEER));
  }

  const float dt = 1.0f / (float)C.sim_freq;
  const int frames = C.sim_freq / C.policy_freq;
  const float a0 = P.actions[2 * (size_t)e], a1 = P.actions[2 * (size_t)e + 1];
  // the road order of the stored positions, kept from the previous step (flags bits 8-13; the
  // absent lanes follow the present ones by descending index), validated -- and repaired or
  // rebuilt when the state was written by someone else -- before frame 0 uses it
  RoadOrder ro;
  ro.rk = lane < V ? order_pos : V + (WAVE - 1 - lane);
  ro.ord = __builtin_amdgcn_ds_permute(ro.rk << 2, lane);
  ro.valid = true;
  const uint64_t pres = ballot(v.present);
  road_order(lane, v, pres, ro);
  float cos_h, sin_h;
  hm_sincosf(v.h, &sin_h, &cos_h);
  SEC(sp, 15);
  if (frames > 0 && lane == 0) {  // ContinuousAction.act (first frame)
    v.aacc = hm_lmap(hm_clipf(a0, -1.0f, 1.0f), -1.0f, 1.0f, -5.0f, 5.0f);
    v.asteer = hm_lmap(hm_clipf(a1, -1.0f, 1.0f), -1.0f, 1.0f, -HM_PIO4_F, HM_PIO4_F);
  }
  // the ego's steering changes only here and to 0 on a crash (handled in frame_wave)
  const float tan_ego = rdlf(lane == 0 ? hm_tanf_sc(v.asteer) : 0.0f, 0);
  // Issue priority falls with progress through the frames (s_setprio 3, 2, 1, 0 from 6/15, 10/15
  // and 13/15 of them): the SIMD's arbiter otherwise prefers its oldest wave, so a SIMD's four
  // waves finished one after another and the last ran its final frames alone, with no other
  // wave to hide its latency.  Lagging waves now catch up and the four finish together (the
  // launch ends with the slowest SIMD).  Scheduling only: the same instructions and results.
  for (int frame = 0; frame < frames; ++frame) {
    const int f15 = 15 * frame;
    if (f15 < 6 * frames) __builtin_amdgcn_s_setprio(3);
    else if (f15 < 10 * frames) __builtin_amdgcn_s_setprio(2);
    else if (f15 < 13 * frames) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
    frame_wave(C, lane, v, dt, tan_ego, ro, cos_h, sin_h, lds_coll[w], sp, pres);
  }
  __builtin_amdgcn_s_setprio(0);  // the reward, observation and stores at the lowest priority
  step += 1;
  SEC(sp, 16);

  // HighwayEnv._reward / _is_terminated / _is_truncated on the ego (lane 0)
  float rew = 0.0f;
  int terminated = 0;
  [[maybe_unused]] float terms[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // INFO: what enters rew
  if (lane == 0) {
    const float forward_speed = v.spd * cos_h;  // hm_cosf(v.h), carried from the last frame
    const float scaled_speed = hm_lmap(forward_speed, C.reward_speed_range[0],
                                       C.reward_speed_range[1], 0.0f, 1.0f);
    const float collision = v.crashed ? 1.0f : 0.0f;
    const int nl = C.lanes_count - 1;
    const float right_lane = (float)v.ln / (float)(nl > 1 ? nl : 1);
    const float high_speed = hm_clipf(scaled_speed, 0.0f, 1.0f);
    const bool on_road = on_lane_m(v.x, v.y, v.ln, 0.0f);
    const float on_road_f = on_road ? 1.0f : 0.0f;
    rew = 0.0f;
    rew = rew + C.collision_reward * collision;
    rew = rew + C.right_lane_reward * right_lane;
    rew = rew + C.high_speed_reward * high_speed;
    rew = rew + C.on_road_reward * on_road_f;
    if (C.normalize_reward)
      rew = hm_lmap(rew, C.collision_reward, C.high_speed_reward + C.right_lane_reward, 0.0f, 1.0f);
    rew = rew * on_road_f;
    terminated = v.crashed || (C.offroad_terminal && !on_road);
    if constexpr (INFO) {
      terms[0] = collision;
      terms[1] = right_lane;
      terms[2] = high_speed;
      terms[3] = on_road_f;
    }
  }
  rew = rdlf(rew, 0);
  terminated = rdli(terminated, 0);
  const int truncated = step >= C.max_steps;
  ep_return = ep_return + rew;
  const bool done = terminated || truncated;
  if (lane == 0) {
    P.reward[e] = rew;
    P.term[e] = (uint8_t)terminated;
    P.trunc[e] = (uint8_t)truncated;
    if (P.ep_ret) P.ep_ret[e] = done ? ep_return : 0.0f;
    if (P.ep_len) P.ep_len[e] = done ? step : 0;
  }
  if constexpr (INFO) {
    // AbstractEnv._info / HighwayEnv._rewards of the ego, and the episode's running sums (the
    // form of ep_return: acc = acc + value in float32, so a host can mirror them exactly)
    if (lane == 0) {
      if (I->speed) I->speed[e] = v.spd;
      if (I->crashed) I->crashed[e] = v.crashed ? 1 : 0;
      if (I->lane) I->lane[e] = v.ln;
      if (I->rewards) {
        float* r = I->rewards + 4 * (size_t)e;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = terms[k];
      }
      if (I->acc) {
        float* a = I->acc + HWY_INFO_NACC * (size_t)e;
        const bool fresh = step == 1;  // step 0 on entry: a new episode's sums start from zero
        const float val[6] = {v.spd, terms[0], terms[1], terms[2], terms[3],
                              v.ln != ln_start ? 1.0f : 0.0f};
        float sum[HWY_INFO_NACC];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const float prev = a[k];
          sum[k] = (fresh ? 0.0f : prev) + val[k];
        }
        sum[6] = sum[7] = 0.0f;
#pragma unroll
        for (int k = 0; k < HWY_INFO_NACC; ++k) a[k] = sum[k];
        if (I->ep_stats) {
          float* es = I->ep_stats + HWY_INFO_NACC * (size_t)e;
          sum[6] = v.crashed ? 1.0f : 0.0f;
#pragma unroll
          for (int k = 0; k < HWY_INFO_NACC; ++k) es[k] = done ? sum[k] : 0.0f;
        }
      }
    }
  }
  SEC(sp, 11);
  if constexpr (FINAL) {
    // the terminal observation (gymnasium's final_observation): what an autoreset-off handle
    // would observe here, from the pre-reset vehicles and this episode's step and seed.  done is
    // wave-uniform and observe_wave's LDS rows are the wave's own, so no barrier is needed.
    if (done && final_obs)
      observe_wave(C, lane, v, cos_h, sin_h, step, seed, group_pe_table(P, e),
                   final_obs + (size_t)e * C.obs_vehicles * P.fout, P.fout, lds_vor[w], lds_inv[w],
                   lds_coll[w].imx);
  }
  if (done && C.autoreset) {
    episode += 1;
    seed = episode_seed(P, e, episode);
    reset_wave(C, lane, seed, v);
    step = 0;
    ep_return = 0.0f;
    ro.rk = reset_order_pos(lane, V);
    cos_h = 1.0f;  // hm_cosf / hm_sinf of the reset heading 0, exactly
    sin_h = 0.0f;
  }
  SEC(sp, 12);
  observe_wave(C, lane, v, cos_h, sin_h, step, seed, group_pe_table(P, e),
               P.obs + (size_t)e * C.obs_vehicles * P.fout, P.fout, lds_vor[w], lds_inv[w],
               lds_coll[w].imx);  // the collision pass's scratch is free after the frames
  SEC(sp, 13);
  store_veh(st, fstride, idx, lane, V, v, ro.rk);
  SEC(sp, 17);
  store_env_words(st, fstride, idx, lane, step, episode, seed, rdlf(v.aacc, 0), rdlf(v.asteer, 0),
                  ep_return);
  SEC(sp, 14);
  WAVE_T(e, lane, 1, __builtin_amdgcn_s_memtime());
  WAVE_T(e, lane, 4, __builtin_amdgcn_s_memrealtime());
  WAVE_T(e, lane, 2, (unsigned long long)done | WAVE_HWID());
  SEC_FLUSH(sp, lane, e);
}

// waves per SIMD the step kernel's registers are sized for at large E (5 and 8 measured slower)
#ifndef HWY_STEP_BIG_W
#define HWY_STEP_BIG_W 6
#endif

// hwy_cut_kernel is compiled as a translation unit of its own from this source (-DHWY_CUT_TU ->
// hwy_cut.o, as ppo_mixed.o / ppo_wide.o are from ppo_kernels.hip): that unit holds the cut
// kernel and its launcher and none of the other kernels, the main unit everything but them, so
// the main unit's code object is the one it was before the cut kernel existed.
#ifdef HWY_CUT_TU
// hwy_cut_episodes: end every running episode (step >= 1) and start the next one of the
// schedule, exactly as step_body's autoreset branch does at a truncation; an env at step 0 is
// left alone (no state or obs store).  One wave per env, as hwy_reset_kernel.
__global__ void __launch_bounds__(256) hwy_cut_kernel(StepParams P, uint8_t* __restrict__ cut) {
  __shared__ int lds_vor[ENVS_PER_BLOCK][WAVE];
  __shared__ int lds_inv[ENVS_PER_BLOCK][WAVE];
  __shared__ unsigned long long lds_key[ENVS_PER_BLOCK][WAVE];
  const hwy_config& C = P.cfg;
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = threadIdx.x / WAVE;
  const int e = blockIdx.x * ENVS_PER_BLOCK + w;
  if (e >= C.num_envs) return;  // whole wave
  const int V = C.vehicles_count + 1;
  const size_t fstride = (size_t)C.num_envs * WAVE;
  const uint32_t idx = (uint32_t)e * WAVE + lane;  // < 2^32: hwy_create bounds num_envs
  const uint32_t ew = (P.state + HWY_F_ENV * fstride)[idx];
  const int step = rdli((int)ew, HWY_E_STEP);
  const int episode = rdli((int)ew, HWY_E_EPISODE) + 1;
  const float ep_return = hm_bits2f((uint32_t)rdli((int)ew, HWY_E_RETURN));
  const bool running = step >= 1;  // wave-uniform
  if (lane == 0) {
    if (cut) cut[e] = running ? 1 : 0;
    if (P.ep_ret) P.ep_ret[e] = running ? ep_return : 0.0f;
    if (P.ep_len) P.ep_len[e] = running ? step : 0;
  }
  if (!running) return;
  const uint64_t seed = episode_seed(P, e, episode);
  Veh v;
  reset_wave(C, lane, seed, v);
  observe_wave(C, lane, v, 1.0f, 0.0f, 0, seed, group_pe_table(P, e),
               P.obs + (size_t)e * C.obs_vehicles * P.fout, P.fout, lds_vor[w], lds_inv[w],
               lds_key[w]);
  store_veh(P.state, fstride, idx, lane, V, v, reset_order_pos(lane, V));
  store_env_words(P.state, fstride, idx, lane, 0, episode, seed, 0.0f, 0.0f, 0.0f);
}

extern "C" int hwy_launch_cut(const StepParams* p, uint8_t* cut, hipStream_t s) {
  const int blocks = (p->cfg.num_envs + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  hipLaunchKernelGGL(hwy_cut_kernel, dim3(blocks), dim3(ENVS_PER_BLOCK * WAVE), 0, s, *p, cut);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#elif defined(HWY_INFO_TU)
// The info variants of the step kernels, likewise a unit of their own (-DHWY_INFO_TU ->
// hwy_info.o): step_body with INFO on, the info pointers a second, separate argument (solo) or a
// second device table (grouped), so StepParams -- the plain kernels' kernarg and table layout --
// is untouched.  Launch geometry and register budgets are the plain kernels'.
template <int W>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, 8)))
hwy_step_info_kernel(StepParams P, InfoParams I) {
  step_body<W, true>(P, &I);
}

template <int W>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, 8)))
hwy_step_grp_info_kernel(const StepParams* __restrict__ tab, const InfoParams* __restrict__ itab) {
  step_body<W, true>(tab[blockIdx.y], itab + blockIdx.y);
}

extern "C" int hwy_launch_step_info(const StepParams* p, const InfoParams* info, hipStream_t s) {
  const int blocks = (p->cfg.num_envs + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  if (hwy_step_big(p->cfg.num_envs))
    hipLaunchKernelGGL(hwy_step_info_kernel<HWY_STEP_BIG_W>, dim3(blocks),
                       dim3(ENVS_PER_BLOCK * WAVE), 0, s, *p, *info);
  else
    hipLaunchKernelGGL(hwy_step_info_kernel<4>, dim3(blocks), dim3(ENVS_PER_BLOCK * WAVE), 0, s,
                       *p, *info);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int hwy_launch_step_group_info(const StepParams* dtab, const InfoParams* itab, int n,
                                          int blocks, int big, hipStream_t s) {
  if (big)
    hipLaunchKernelGGL(hwy_step_grp_info_kernel<HWY_STEP_BIG_W>, dim3(blocks, n),
                       dim3(ENVS_PER_BLOCK * WAVE), 0, s, dtab, itab);
  else
    hipLaunchKernelGGL(hwy_step_grp_info_kernel<4>, dim3(blocks, n), dim3(ENVS_PER_BLOCK * WAVE),
                       0, s, dtab, itab);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#elif defined(HWY_FINAL_TU)
// The final variants of the step kernels and hwy_gae_boot's kernel, likewise a unit of their own
// (-DHWY_FINAL_TU -> hwy_final.o): step_body with INFO and FINAL on, the (nullable) info
// pointers and the final observation's buffer a second argument (solo) or a second device table
// (grouped).  Launch geometry and register budgets are the plain kernels'.
template <int W>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, 8)))
hwy_step_final_kernel(StepParams P, FinalParams F) {
  step_body<W, true, true>(P, &F.info, F.final_obs);
}

template <int W>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, 8)))
hwy_step_grp_final_kernel(const StepParams* __restrict__ tab,
                          const FinalParams* __restrict__ ftab) {
  const FinalParams* F = ftab + blockIdx.y;
  step_body<W, true, true>(tab[blockIdx.y], &F->info, F->final_obs);
}

extern "C" int hwy_launch_step_final(const StepParams* p, const FinalParams* f, hipStream_t s) {
  const int blocks = (p->cfg.num_envs + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  if (hwy_step_big(p->cfg.num_envs))
    hipLaunchKernelGGL(hwy_step_final_kernel<HWY_STEP_BIG_W>, dim3(blocks),
                       dim3(ENVS_PER_BLOCK * WAVE), 0, s, *p, *f);
  else
    hipLaunchKernelGGL(hwy_step_final_kernel<4>, dim3(blocks), dim3(ENVS_PER_BLOCK * WAVE), 0, s,
                       *p, *f);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int hwy_launch_step_group_final(const StepParams* dtab, const FinalParams* ftab, int n,
                                           int blocks, int big, hipStream_t s) {
  if (big)
    hipLaunchKernelGGL(hwy_step_grp_final_kernel<HWY_STEP_BIG_W>, dim3(blocks, n),
                       dim3(ENVS_PER_BLOCK * WAVE), 0, s, dtab, ftab);
  else
    hipLaunchKernelGGL(hwy_step_grp_final_kernel<4>, dim3(blocks, n), dim3(ENVS_PER_BLOCK * WAVE),
                       0, s, dtab, ftab);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// hwy_gae_kernel with a bootstrap at truncation: a truncated, not terminated row takes
// boot[i] = V(final observation) as its next-state value and the chain is cut there.  With no
// such row every expression below is hwy_gae_kernel's, operation for operation.
__global__ void __launch_bounds__(64) hwy_gae_boot_kernel(const float* __restrict__ rew,
                                                           const uint8_t* __restrict__ term,
                                                           const uint8_t* __restrict__ trunc,
                                                           const float* __restrict__ val,
                                                           const float* __restrict__ last_val,
                                                           const float* __restrict__ bootv,
                                                           double gamma, double lam, int T, int E,
                                                           float* __restrict__ adv,
                                                           float* __restrict__ ret) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const double gl = gamma * lam;
  float last_adv = 0.0f;
  double v1 = (double)last_val[e];
  constexpr int kGaeAhead = 8;  // as hwy_gae_kernel: the loads of 8 steps go ahead of their use
  for (int t1 = T; t1 > 0; t1 -= kGaeAhead) {
    float rv[kGaeAhead], vv[kGaeAhead], bv[kGaeAhead];
    uint8_t tm[kGaeAhead], tr[kGaeAhead];
#pragma unroll
    for (int j = 0; j < kGaeAhead; ++j) {
      const int t = t1 - 1 - j;
      const size_t i = (size_t)(t < 0 ? 0 : t) * E + e;
      rv[j] = rew[i], vv[j] = val[i], bv[j] = bootv[i], tm[j] = term[i], tr[j] = trunc[i];
    }
#pragma unroll
    for (int j = 0; j < kGaeAhead; ++j) {
      const int t = t1 - 1 - j;
      if (t < 0) break;
      const size_t i = (size_t)t * E + e;
      const float v0f = vv[j];
      const bool done = tm[j] | tr[j];
      const bool boot = tr[j] && !tm[j];
      const double vsel = boot ? (double)bv[j] : v1;
      const double m = (done && !boot) ? 0.0 : 1.0;
      const double nd = done ? 0.0 : 1.0;
      const double delta = ((double)rv[j] + (gamma * vsel) * m) - (double)v0f;
      const float a = (float)(delta + (gl * nd) * (double)last_adv);
      adv[i] = a;
      ret[i] = a + v0f;
      last_adv = a;
      v1 = (double)v0f;
    }
  }
}

extern "C" int hwy_launch_gae_boot(const float* rew, const uint8_t* term, const uint8_t* trunc,
                                   const float* val, const float* last_val, const float* bootv,
                                   double gamma, double lam, int T, int E, float* adv, float* ret,
                                   hipStream_t s) {
  if (E == 0) return 0;
  const int blocks = (E + 63) / 64;
  hipLaunchKernelGGL(hwy_gae_boot_kernel, dim3(blocks), dim3(64), 0, s, rew, term, trunc, val,
                     last_val, bootv, gamma, lam, T, E, adv, ret);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#elif defined(HWY_OBSERVE_TU)
// hwy_observe's kernel, likewise a unit of its own (-DHWY_OBSERVE_TU -> hwy_observe.o): the
// observation of the stored state, through the step's own observe_wave (its MAP instantiation,
// which exists in this unit only), with the row -> vehicle map and the scatter of per-row values
// to per-vehicle ones.  One wave per env, lane = vehicle, as the step; it loads the five fields
// the observation reads (x, y, heading, speed, flags) and the env words, 1,536 B per env, and
// writes nothing but its outputs.  P.p.cfg.order is the order the call asked for.
__global__ void __launch_bounds__(256) hwy_observe_kernel(ObserveParams P) {
  __shared__ int lds_vor[ENVS_PER_BLOCK][WAVE];
  __shared__ int lds_inv[ENVS_PER_BLOCK][WAVE];
  __shared__ unsigned long long lds_key[ENVS_PER_BLOCK][WAVE];
  __shared__ uint32_t lds_val[ENVS_PER_BLOCK][WAVE];
  const hwy_config& C = P.p.cfg;
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = threadIdx.x / WAVE;
  const int e = blockIdx.x * ENVS_PER_BLOCK + w;
  if (e >= C.num_envs) return;  // whole wave
  const int V = C.vehicles_count + 1;
  const int N = C.obs_vehicles;
  const size_t fstride = (size_t)C.num_envs * WAVE;
  const uint32_t idx = (uint32_t)e * WAVE + lane;  // < 2^32: hwy_create bounds num_envs
  const uint32_t* st = P.p.state;
  Veh v{};  // the fields the observation does not read stay zero
  v.x = hm_bits2f((st + HWY_F_X * fstride)[idx]);
  v.y = hm_bits2f((st + HWY_F_Y * fstride)[idx]);
  v.h = hm_bits2f((st + HWY_F_HEADING * fstride)[idx]);
  v.spd = hm_bits2f((st + HWY_F_SPEED * fstride)[idx]);
  const uint32_t fl = (st + HWY_F_FLAGS * fstride)[idx];
  const uint32_t ew = (st + HWY_F_ENV * fstride)[idx];
  v.present = ((fl & HWY_FLAG_PRESENT) != 0u) && lane < V;  // load_veh's rule
  const int step = rdli((int)ew, HWY_E_STEP);
  const uint64_t seed = (uint64_t)(uint32_t)rdli((int)ew, HWY_E_SEED_LO) |
                        ((uint64_t)(uint32_t)rdli((int)ew, HWY_E_SEED_HI) << 32);
  float cos_h, sin_h;
  hm_sincosf(v.h, &sin_h, &cos_h);
  int rv;
  observe_wave<true>(C, lane, v, cos_h, sin_h, step, seed, group_pe_table(P.p, e),
                     P.p.obs ? P.p.obs + (size_t)e * N * P.p.fout : nullptr, P.p.fout, lds_vor[w],
                     lds_inv[w], lds_key[w], &rv);
  if (P.row_vehicle && lane < N) P.row_vehicle[(size_t)e * N + lane] = rv;
  if (P.veh_values) {
    // the scatter in LDS, zeros first and the rows after a wave barrier, then one coalesced
    // store of the env's 64 words: every entry is written exactly once
    const uint32_t bits = (lane < N && rv >= 0) ? hm_f2bits(P.row_values[(size_t)e * N + lane]) : 0u;
    lds_val[w][lane] = 0u;
    wave_lds_sync();
    if (lane < N && rv >= 0) lds_val[w][rv] = bits;  // rv in 0..63, distinct over the rows
    wave_lds_sync();
    ((uint32_t*)P.veh_values)[idx] = lds_val[w][lane];
  }
}

extern "C" int hwy_launch_observe(const ObserveParams* p, hipStream_t s) {
  const int blocks = (p->p.cfg.num_envs + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  hipLaunchKernelGGL(hwy_observe_kernel, dim3(blocks), dim3(ENVS_PER_BLOCK * WAVE), 0, s, *p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#elif defined(HWY_TRAFFIC_TU)
// hwy_traffic's kernel, likewise a unit of its own (-DHWY_TRAFFIC_TU -> hwy_traffic.o): the
// neighbours of every vehicle through the step's own road_order / lane_scan /
// neighbours_ordered, and from them the gap, time-to-collision and headway of include/hwy.h, the
// ego row and the running per-episode reduction.  One wave per env, lane = vehicle, as the step;
// it loads six fields (x, y, heading, speed, lane, flags), 1,536 B per env, and writes nothing
// but the outputs it was given.  Every cross-lane read runs with all 64 lanes active; the
// per-lane index of a gather is a road-order entry or the lane itself, so it is in 0..63.

// 0 where gap <= 0, else gap / den where den > 0, else +inf (ttc: den = closing; thw: den = vx)
__device__ __forceinline__ float gap_over(float gap, float den) {
  return gap <= 0.0f ? 0.0f : (den > 0.0f ? gap / den : hm_bits2f(0x7f800000u));
}

__global__ void __launch_bounds__(256) hwy_traffic_kernel(TrafficParams P) {
  const hwy_config& C = P.cfg;
  const hwy_traffic_args& A = P.a;
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = threadIdx.x / WAVE;
  const int e = blockIdx.x * ENVS_PER_BLOCK + w;
  if (e >= C.num_envs) return;  // whole wave
  const int V = C.vehicles_count + 1;
  const size_t fstride = (size_t)C.num_envs * WAVE;
  const uint32_t idx = (uint32_t)e * WAVE + lane;  // < 2^32: hwy_create bounds num_envs
  const uint32_t* st = P.state;
  const float inf = hm_bits2f(0x7f800000u);
  Veh v{};  // the fields the neighbour search does not read stay zero
  v.x = hm_bits2f((st + HWY_F_X * fstride)[idx]);
  v.y = hm_bits2f((st + HWY_F_Y * fstride)[idx]);
  v.h = hm_bits2f((st + HWY_F_HEADING * fstride)[idx]);
  v.spd = hm_bits2f((st + HWY_F_SPEED * fstride)[idx]);
  v.ln = (int)(st + HWY_F_LANE * fstride)[idx];
  const uint32_t fl = (st + HWY_F_FLAGS * fstride)[idx];
  v.present = ((fl & HWY_FLAG_PRESENT) != 0u) && lane < V;  // load_veh's rule
  const uint64_t pres = ballot(v.present);

  // Road.neighbour_vehicles on lanes ln - 1, ln, ln + 1 (slot s <-> lane ln - 1 + s), as
  // frame_wave asks for them
  RoadOrder ro;
  ro.rk = 0;
  ro.ord = 0;
  ro.valid = false;
  road_order(lane, v, pres, ro);
  const float xq = shf(v.x, ro.ord);
  int fi[3], ri[3], qfp[3];
  neighbours_ordered(C, lane, v, pres, ro, xq, fi, ri, qfp);

  float sin_h, cos_h;
  hm_sincosf(v.h, &sin_h, &cos_h);
  const float vx = v.spd * cos_h;

  // gaps towards the front / the rear of slot s: (x_f - x_i) - 5 and (x_i - x_r) - 5, +inf for none
  float fgap[3], rgap[3];
  bool hasf[3], hasr[3];
  float vxf = 0.0f, vxr = 0.0f;  // vx of the own lane's front / rear (this vehicle's without one)
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    hasf[s] = v.present && fi[s] >= 0;
    hasr[s] = v.present && ri[s] >= 0;
    const int fsrc = hasf[s] ? fi[s] : lane, rsrc = hasr[s] ? ri[s] : lane;
    const float xf = shf(v.x, fsrc), xr = shf(v.x, rsrc);
    fgap[s] = hasf[s] ? (xf - v.x) - VEH_LENGTH : inf;
    rgap[s] = hasr[s] ? (v.x - xr) - VEH_LENGTH : inf;
    if (s == 1) {
      vxf = shf(vx, fsrc);
      vxr = shf(vx, rsrc);
    }
  }
  const float gap = fgap[1];
  const float closing = hasf[1] ? vx - vxf : 0.0f;
  const float ttc = v.present ? gap_over(gap, closing) : inf;
  const float thw = v.present ? gap_over(gap, vx) : inf;
  const float risk = ttc < A.risk_horizon ? 1.0f - ttc / A.risk_horizon : 0.0f;
  if (A.front) A.front[idx] = hasf[1] ? fi[1] : -1;
  if (A.rear) A.rear[idx] = hasr[1] ? ri[1] : -1;
  if (A.gap) A.gap[idx] = gap;
  if (A.closing) A.closing[idx] = closing;
  if (A.ttc) A.ttc[idx] = ttc;
  if (A.thw) A.thw[idx] = thw;
  if (A.risk) A.risk[idx] = risk;
  if (!A.ego && !A.acc) return;  // wave-uniform

  // ---- the ego row: vehicle 0's values, broadcast, lane s of the first 16 holding slot s
  const float rclos = hasr[1] ? vxr - vx : 0.0f;
  const float rttc = gap_over(rgap[1], rclos);
  const float ex = rdlf(v.x, 0), ey = rdlf(v.y, 0);
  const float dx = v.x - ex, dy = v.y - ey;
  const bool other = v.present && lane != 0;
  // the least dx*dx + dy*dy as the greatest of the negated squares (exact either way)
  const float dist = __builtin_sqrtf(-wave_max_f(other ? -(dx * dx + dy * dy) : -inf));
  const uint64_t nearm = ballot(other) & ballot(0.0f <= dx) & ballot(dx <= A.near_range);
  const float off = lane_lat(v.y, v.ln);
  const float gap0 = rdlf(gap, 0), ttc0 = rdlf(ttc, 0), thw0 = rdlf(thw, 0);
  const float slot[HWY_TRAFFIC_NEGO] = {
      gap0, rdlf(closing, 0), ttc0, thw0, rdlf(rgap[1], 0), rdlf(rclos, 0), rdlf(rttc, 0),
      rdlf(fgap[0], 0), rdlf(rgap[0], 0), rdlf(fgap[2], 0), rdlf(rgap[2], 0), dist,
      (float)__popcll(nearm), rdlf(off, 0), rdlf(vx, 0), rdlf(risk, 0)};
  if (A.ego) {
    float ev = 0.0f;
#pragma unroll
    for (int s = 0; s < HWY_TRAFFIC_NEGO; ++s) ev = lane == s ? slot[s] : ev;
    if (lane < HWY_TRAFFIC_NEGO) A.ego[(size_t)e * HWY_TRAFFIC_NEGO + lane] = ev;
  }
  if (!A.acc) return;

  // ---- the running reduction: lane s of the first 8 holds slot s of the env's row
  bool restart = false;  // wave-uniform
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (A.restart[k]) restart = restart || A.restart[k][e] != 0;
  const float one_if_front = rdli((int)hasf[1], 0) ? 1.0f : 0.0f;
  const float now[HWY_TRAFFIC_NACC] = {1.0f, ttc0, thw0, gap0, dist,
                                       ttc0 < A.ttc_thresh ? 1.0f : 0.0f,
                                       thw0 < A.thw_thresh ? 1.0f : 0.0f, one_if_front};
  float sv = 0.0f;
#pragma unroll
  for (int s = 0; s < HWY_TRAFFIC_NACC; ++s) sv = lane == s ? now[s] : sv;
  const bool mine = lane < HWY_TRAFFIC_NACC;
  const size_t ai = (size_t)e * HWY_TRAFFIC_NACC + (mine ? lane : 0);
  const float old = mine ? A.acc[ai] : 0.0f;
  const bool fresh = restart || rdlf(old, 0) == 0.0f;
  const bool is_min = lane >= 1 && lane <= 4;
  const float merged = is_min ? hm_minf(old, sv) : old + sv;
  if (mine) {
    A.acc[ai] = fresh ? sv : merged;
    if (A.ep_stats) A.ep_stats[ai] = restart ? old : 0.0f;
  }
}

extern "C" int hwy_launch_traffic(const TrafficParams* p, hipStream_t s) {
  const int blocks = (p->cfg.num_envs + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  hipLaunchKernelGGL(hwy_traffic_kernel, dim3(blocks), dim3(ENVS_PER_BLOCK * WAVE), 0, s, *p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#elif defined(HWY_SENSE_TU)
// hwy_sense's kernel, likewise a unit of its own (-DHWY_SENSE_TU -> hwy_sense.o): the sensor
// model of include/hwy.h as a front end to the step's own observe_wave (its MAP instantiation, as
// in the observe unit), which is handed a perceived copy of the vehicles: not visible -> not
// present, x / y / speed perturbed.  One wave per env, lane = vehicle, as the step; it loads the
// five fields the observation reads and the env words, 1,536 B per env, and writes nothing but
// the outputs it was given.  Every cross-lane operation runs with all 64 lanes active; the
// branches around the line-of-sight loop, the draws and the observation are wave-uniform.

// one Philox draw of the sensor's stream: counter (vehicle, step word, channel, salt word)
__device__ __forceinline__ hm_u32x4 sense_draw(int lane, int step, uint32_t ch, uint32_t salt_word,
                                               uint64_t seed) {
  return hm_philox4x32_10((uint32_t)lane, (uint32_t)step, ch, salt_word,
                          (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
}

// the unit-variance draw of channel ch: four uniforms summed pairwise, centred and scaled
__device__ __forceinline__ float sense_z(int lane, int step, uint32_t ch, uint32_t salt_word,
                                         uint64_t seed) {
  const hm_u32x4 w = sense_draw(lane, step, ch, salt_word, seed);
  const float u0 = hm_u01(w.v[0]), u1 = hm_u01(w.v[1]), u2 = hm_u01(w.v[2]), u3 = hm_u01(w.v[3]);
  return (((u0 + u1) + (u2 + u3)) - 2.0f) * 1.7320508f;
}

__global__ void __launch_bounds__(256) hwy_sense_kernel(SenseParams P) {
  __shared__ int lds_vor[ENVS_PER_BLOCK][WAVE];
  __shared__ int lds_inv[ENVS_PER_BLOCK][WAVE];
  __shared__ unsigned long long lds_key[ENVS_PER_BLOCK][WAVE];
  // the blockers' image: (x, y, cos h, sin h) and the ego's centre in the blocker's frame
  __shared__ float4 lds_body[ENVS_PER_BLOCK][WAVE];
  __shared__ float2 lds_ego[ENVS_PER_BLOCK][WAVE];
  const hwy_config& C = P.p.cfg;
  const hwy_sense_args& A = P.a;
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = threadIdx.x / WAVE;
  const int e = blockIdx.x * ENVS_PER_BLOCK + w;
  if (e >= C.num_envs) return;  // whole wave
  const int V = C.vehicles_count + 1;
  const int N = C.obs_vehicles;
  const size_t fstride = (size_t)C.num_envs * WAVE;
  const uint32_t idx = (uint32_t)e * WAVE + lane;  // < 2^32: hwy_create bounds num_envs
  const uint32_t* st = P.p.state;
  Veh v{};  // the fields the observation does not read stay zero
  v.x = hm_bits2f((st + HWY_F_X * fstride)[idx]);
  v.y = hm_bits2f((st + HWY_F_Y * fstride)[idx]);
  v.h = hm_bits2f((st + HWY_F_HEADING * fstride)[idx]);
  v.spd = hm_bits2f((st + HWY_F_SPEED * fstride)[idx]);
  const uint32_t fl = (st + HWY_F_FLAGS * fstride)[idx];
  const uint32_t ew = (st + HWY_F_ENV * fstride)[idx];
  v.present = ((fl & HWY_FLAG_PRESENT) != 0u) && lane < V;  // load_veh's rule
  const int step = rdli((int)ew, HWY_E_STEP);
  const uint64_t seed = (uint64_t)(uint32_t)rdli((int)ew, HWY_E_SEED_LO) |
                        ((uint64_t)(uint32_t)rdli((int)ew, HWY_E_SEED_HI) << 32);
  float cos_h, sin_h;
  hm_sincosf(v.h, &sin_h, &cos_h);

  // ---- visibility, on the true positions
  const float ex = rdlf(v.x, 0), ey = rdlf(v.y, 0);
  const bool other = v.present && lane >= 1;
  const uint64_t otherm = ballot(other);
  const float dx = v.x - ex, dy = v.y - ey;
  const float d2 = dx * dx + dy * dy;
  const bool in_range = d2 <= P.range2;
  bool blocked = false;
  if (A.los) {
    // Only an in-range vehicle's blocked bit reaches an output, and its sight segment lies inside
    // the range circle.  A body whose centre is more than (range_m + 4 m) * 1.0001 from the ego
    // (its half diagonal is 2.7 m) has no point within a metre of that circle, so it cannot meet such a
    // segment and is left out of the loop: wave-uniformly, and never with range_m = +inf
    // (cull2 = +inf) or a NaN distance (the comparison is false).
    const uint64_t bodym = otherm & ~ballot(d2 > P.cull2);
    // lane j lays out its body and the ego's centre in its frame (u0, w0: the same for every k);
    // lane k then reads blocker j's six words at one address (broadcast)
    const float ax = ex - v.x, ay = ey - v.y;
    lds_body[w][lane] = make_float4(v.x, v.y, cos_h, sin_h);
    lds_ego[w][lane] = make_float2(ax * cos_h + ay * sin_h, ay * cos_h - ax * sin_h);
    wave_lds_sync();
    for (int j = 1; j < V; ++j) {
      if (!((bodym >> j) & 1ull)) continue;  // wave-uniform: an absent slot is no body
      const float4 b = lds_body[w][j];
      const float2 eo = lds_ego[w][j];
      const float u0 = eo.x, w0 = eo.y;
      const float bx = v.x - b.x, by = v.y - b.y;
      const float u1 = bx * b.z + by * b.w;
      const float w1 = by * b.z - bx * b.w;
      const bool hit = hm_minf(u0, u1) <= 0.5f * VEH_LENGTH && hm_maxf(u0, u1) >= -0.5f * VEH_LENGTH &&
                       hm_minf(w0, w1) <= 0.5f * VEH_WIDTH && hm_maxf(w0, w1) >= -0.5f * VEH_WIDTH &&
                       hm_absf(u0 * w1 - u1 * w0) <= (0.5f * VEH_LENGTH) * hm_absf(w1 - w0) +
                                                         (0.5f * VEH_WIDTH) * hm_absf(u1 - u0);
      blocked = blocked || (hit && j != lane);
    }
  }
  bool dropped = false;
  if (A.p_drop > 0.0f)  // u < 0 never holds
    dropped = hm_u01(sense_draw(lane, step, 3u, P.salt_word, seed).v[0]) < A.p_drop;
  const bool visible = lane == 0 ? v.present : (other && in_range && !blocked && !dropped);

  if (A.visible) A.visible[idx] = visible ? 1 : 0;
  if (A.hidden) A.hidden[idx] = (v.present && !visible) ? 1.0f : 0.0f;
  if (A.counts) {
    const uint64_t outm = ballot(other && !in_range);
    const uint64_t blkm = ballot(other && in_range && blocked);
    const uint64_t drpm = ballot(other && in_range && !blocked && dropped);
    int cv = __popcll(otherm);
    cv = lane == 1 ? __popcll(outm) : cv;
    cv = lane == 2 ? __popcll(blkm) : cv;
    cv = lane == 3 ? __popcll(drpm) : cv;
    if (lane < 4) A.counts[(size_t)e * 4 + lane] = cv;
  }

  // ---- the observation of the perceived vehicles
  if (P.p.obs || A.row_vehicle) {  // wave-uniform
    Veh pv = v;
    pv.present = v.present && visible;
    // a sigma of exactly 0 skips its addition; the ego is never perturbed
    if (A.sigma[0] != 0.0f) {
      const float z = sense_z(lane, step, 0u, P.salt_word, seed);
      if (lane >= 1) pv.x = v.x + A.sigma[0] * z;
    }
    if (A.sigma[1] != 0.0f) {
      const float z = sense_z(lane, step, 1u, P.salt_word, seed);
      if (lane >= 1) pv.y = v.y + A.sigma[1] * z;
    }
    if (A.sigma[2] != 0.0f) {
      const float z = sense_z(lane, step, 2u, P.salt_word, seed);
      if (lane >= 1) pv.spd = v.spd + A.sigma[2] * z;
    }
    int rv;
    observe_wave<true>(C, lane, pv, cos_h, sin_h, step, seed, group_pe_table(P.p, e),
                       P.p.obs ? P.p.obs + (size_t)e * N * P.p.fout : nullptr, P.p.fout,
                       lds_vor[w], lds_inv[w], lds_key[w], &rv);
    if (A.row_vehicle && lane < N) A.row_vehicle[(size_t)e * N + lane] = rv;
  }
}

extern "C" int hwy_launch_sense(const SenseParams* p, hipStream_t s) {
  const int blocks = (p->p.cfg.num_envs + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  hipLaunchKernelGGL(hwy_sense_kernel, dim3(blocks), dim3(ENVS_PER_BLOCK * WAVE), 0, s, *p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#elif defined(HWY_LOOKAHEAD_TU)
// hwy_lookahead's kernels, likewise a unit of their own (-DHWY_LOOKAHEAD_TU -> hwy_lookahead.o):
// K what-if rollouts per env from the stored state, through the step's own load_veh, road_order,
// frame_wave and observe_wave.  One wave per (env, candidate), lane = vehicle, four waves per
// workgroup as the step.  A branch is what hwy_step does on an autoreset-off handle, H times or
// until the first done step, with the state kept in registers: between two steps the vehicles go
// through the image of store_veh / load_veh (the words a step stores and the next one loads), so
// every step starts from exactly what a stored state would have given it.  Nothing is written
// but the outputs; store_veh is never called.  `done` is wave-uniform: the early exit needs no
// barrier, and every cross-lane operation runs with all 64 lanes active.

// the "not run" values of branch b (lazy: its env's candidate 0 did not terminate)
__device__ __forceinline__ void lookahead_not_run(const hwy_lookahead_args& A, int lane, size_t b,
                                                  int H, int nobs) {
  if (lane == 0) {
    if (A.steps) A.steps[b] = 0;
    if (A.terminated) A.terminated[b] = 0;
    if (A.truncated) A.truncated[b] = 0;
    if (A.ret) A.ret[b] = 0.0f;
  }
  if (A.rewards && lane < H) A.rewards[b * H + lane] = 0.0f;  // H <= 64
  if (A.ego_final && lane < 4) A.ego_final[b * 4 + lane] = 0.0f;
  if (A.obs)
    for (int i = lane; i < nobs; i += WAVE) A.obs[b * nobs + i] = 0.0f;
}

// W: waves per SIMD the registers are sized for, as the step's kernels and picked as they are (4,
// or HWY_STEP_BIG_W above 32 waves per CU: at 16,384 / 24,576 waves the 6-wave build takes 857 /
// 1,608 us against the 4-wave build's 917 / 1,776, profiles/r20/lookahead).  This launch runs
// candidates k0 .. k0 + nk - 1 of every env; gate: a wave first reads terminated[e][0] (written by
// an earlier launch on the stream) and writes the "not run" values when it is 0.
template <int W>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, 8)))
hwy_lookahead_kernel(LookaheadParams P) {
  __shared__ int lds_vor[ENVS_PER_BLOCK][WAVE];
  __shared__ int lds_inv[ENVS_PER_BLOCK][WAVE];
  __shared__ CollLds lds_coll[ENVS_PER_BLOCK];
  const hwy_config& C = P.p.cfg;
  const hwy_lookahead_args& A = P.a;
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = threadIdx.x / WAVE;
  const int wi = blockIdx.x * ENVS_PER_BLOCK + w;  // < E * K <= 2^22
  if (wi >= C.num_envs * P.nk) return;             // whole wave
  const int e = wi / P.nk;
  const int k = P.k0 + (wi - e * P.nk);
  const int K = A.k, H = A.horizon;
  const size_t b = (size_t)e * K + k;
  const int V = C.vehicles_count + 1;
  const int nobs = C.obs_vehicles * P.p.fout;
  if (P.gate && A.terminated[(size_t)e * K] == 0) {  // wave-uniform
    lookahead_not_run(A, lane, b, H, nobs);
    return;
  }
  const size_t fstride = (size_t)C.num_envs * WAVE;
  const uint32_t idx = (uint32_t)e * WAVE + lane;  // < 2^32: hwy_create bounds num_envs
  const uint32_t* st = P.p.state;

  SecProf sp;
  SEC_START(sp);
  Veh v;
  int order_pos;
  load_veh(st, fstride, idx, lane, V, v, order_pos);
  const uint32_t ew = (st + HWY_F_ENV * fstride)[idx];
  int step = rdli((int)ew, HWY_E_STEP);
  const uint64_t seed = (uint64_t)(uint32_t)rdli((int)ew, HWY_E_SEED_LO) |
                        ((uint64_t)(uint32_t)rdli((int)ew, HWY_E_SEED_HI) << 32);
  if (lane == 0) {
    v.aacc = hm_bits2f((uint32_t)rdli((int)ew, HWY_E_EGO_ACC));
    v.asteer = hm_bits2f((uint32_t)rdli((int)ew, HWY_E_EGO_STEER));
  }
  const float dt = 1.0f / (float)C.sim_freq;
  const int frames = C.sim_freq / C.policy_freq;
  const float* act = A.actions + (A.hold ? b * 2 : b * (size_t)H * 2);

  RoadOrder ro;
  ro.rk = order_pos;
  float cos_h = 1.0f, sin_h = 0.0f;
  float ret = 0.0f, g = 1.0f;
  int terminated = 0, truncated = 0, n = 0;
  for (int h = 0; h < H; ++h) {
    if (h > 0) {
      // what store_veh writes and load_veh reads back: a slot past V holds zero words, the
      // impact of a vehicle without the impact flag is zero, only the ego's action persists
      const bool live = lane < V;
      v.x = live ? v.x : 0.0f;
      v.y = live ? v.y : 0.0f;
      v.h = live ? v.h : 0.0f;
      v.spd = live ? v.spd : 0.0f;
      v.tsp = live ? v.tsp : 0.0f;
      v.dlt = live ? v.dlt : 0.0f;
      v.tmr = live ? v.tmr : 0.0f;
      v.ix = (live && v.imp) ? v.ix : 0.0f;
      v.iy = (live && v.imp) ? v.iy : 0.0f;
      v.ln = live ? v.ln : 0;
      v.tl = live ? v.tl : 0;
      v.crashed = live && v.crashed;
      v.imp = live && v.imp;
      v.present = live && v.present;
      if (lane != 0) {
        v.aacc = 0.0f;
        v.asteer = 0.0f;
      }
    }
    const float a0 = act[A.hold ? 0 : 2 * h], a1 = act[A.hold ? 1 : 2 * h + 1];
    // the road order kept from the previous step, validated as step_body does
    ro.rk = lane < V ? ro.rk : V + (WAVE - 1 - lane);
    ro.ord = __builtin_amdgcn_ds_permute(ro.rk << 2, lane);
    ro.valid = true;
    const uint64_t pres = ballot(v.present);
    road_order(lane, v, pres, ro);
    hm_sincosf(v.h, &sin_h, &cos_h);
    if (frames > 0 && lane == 0) {  // ContinuousAction.act (first frame)
      v.aacc = hm_lmap(hm_clipf(a0, -1.0f, 1.0f), -1.0f, 1.0f, -5.0f, 5.0f);
      v.asteer = hm_lmap(hm_clipf(a1, -1.0f, 1.0f), -1.0f, 1.0f, -HM_PIO4_F, HM_PIO4_F);
    }
    const float tan_ego = rdlf(lane == 0 ? hm_tanf_sc(v.asteer) : 0.0f, 0);
    for (int frame = 0; frame < frames; ++frame) {  // the step's priority ladder
      const int f15 = 15 * frame;
      if (f15 < 6 * frames) __builtin_amdgcn_s_setprio(3);
      else if (f15 < 10 * frames) __builtin_amdgcn_s_setprio(2);
      else if (f15 < 13 * frames) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
      frame_wave(C, lane, v, dt, tan_ego, ro, cos_h, sin_h, lds_coll[w], sp, pres);
    }
    __builtin_amdgcn_s_setprio(0);
    step += 1;

    // HighwayEnv._reward / _is_terminated / _is_truncated on the ego: step_body's expressions
    float rew = 0.0f;
    terminated = 0;
    if (lane == 0) {
      const float forward_speed = v.spd * cos_h;
      const float scaled_speed = hm_lmap(forward_speed, C.reward_speed_range[0],
                                         C.reward_speed_range[1], 0.0f, 1.0f);
      const float collision = v.crashed ? 1.0f : 0.0f;
      const int nl = C.lanes_count - 1;
      const float right_lane = (float)v.ln / (float)(nl > 1 ? nl : 1);
      const float high_speed = hm_clipf(scaled_speed, 0.0f, 1.0f);
      const bool on_road = on_lane_m(v.x, v.y, v.ln, 0.0f);
      const float on_road_f = on_road ? 1.0f : 0.0f;
      rew = 0.0f;
      rew = rew + C.collision_reward * collision;
      rew = rew + C.right_lane_reward * right_lane;
      rew = rew + C.high_speed_reward * high_speed;
      rew = rew + C.on_road_reward * on_road_f;
      if (C.normalize_reward)
        rew = hm_lmap(rew, C.collision_reward, C.high_speed_reward + C.right_lane_reward, 0.0f, 1.0f);
      rew = rew * on_road_f;
      terminated = v.crashed || (C.offroad_terminal && !on_road);
    }
    rew = rdlf(rew, 0);
    terminated = rdli(terminated, 0);
    truncated = step >= C.max_steps;
    const float gr = g * rew;  // rounded before the sum (no contraction in this unit)
    ret = ret + gr;
    g = g * A.gamma;
    if (A.rewards && lane == 0) A.rewards[b * H + h] = rew;
    n = h + 1;
    if (terminated || truncated) break;  // wave-uniform
  }
  if (A.rewards && lane >= n && lane < H) A.rewards[b * H + lane] = 0.0f;
  if (lane == 0) {
    if (A.steps) A.steps[b] = n;
    if (A.terminated) A.terminated[b] = (uint8_t)terminated;
    if (A.truncated) A.truncated[b] = (uint8_t)truncated;
    if (A.ret) A.ret[b] = ret;
    if (A.ego_final) {
      float* o = A.ego_final + b * 4;
      o[0] = v.x;
      o[1] = v.y;
      o[2] = v.h;
      o[3] = v.spd;
    }
  }
  if (A.obs)  // wave-uniform; the collision pass's scratch is free after the frames
    observe_wave(C, lane, v, cos_h, sin_h, step, seed, group_pe_table(P.p, e), A.obs + b * nobs,
                 P.p.fout, lds_vor[w], lds_inv[w], lds_coll[w].imx);
}

// the shield's choice, one thread per env: the least k with terminated 0; if there is none the k
// with the most steps, the least such k on ties.  Under lazy a skipped candidate holds steps 0
// and terminated 0 only when candidate 0 is safe, which is then chosen first anyway.
__global__ void __launch_bounds__(256) hwy_lookahead_choice_kernel(LookaheadParams P) {
  const hwy_lookahead_args& A = P.a;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= P.p.cfg.num_envs) return;
  const int K = A.k;
  const size_t b0 = (size_t)e * K;
  int best = -1, best_steps = -1, pick = -1;
  for (int k = 0; k < K; ++k) {
    if (A.terminated[b0 + k] == 0) {
      pick = k;
      break;
    }
    const int s = A.steps[b0 + k];
    if (s > best_steps) {
      best_steps = s;
      best = k;
    }
  }
  if (pick < 0) pick = best;
  A.chosen[e] = pick;
  if (A.chosen_action) {
    const uint32_t* src = (const uint32_t*)A.actions +
                          (A.hold ? (b0 + pick) * 2 : (b0 + pick) * (size_t)A.horizon * 2);
    uint32_t* dst = (uint32_t*)A.chosen_action + (size_t)e * 2;
    dst[0] = src[0];
    dst[1] = src[1];
  }
}

extern "C" int hwy_launch_lookahead(const LookaheadParams* p, int big, hipStream_t s) {
  const long waves = (long)p->p.cfg.num_envs * p->nk;
  const int blocks = (int)((waves + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK);
  if (big)
    hipLaunchKernelGGL(hwy_lookahead_kernel<HWY_STEP_BIG_W>, dim3(blocks),
                       dim3(ENVS_PER_BLOCK * WAVE), 0, s, *p);
  else
    hipLaunchKernelGGL(hwy_lookahead_kernel<4>, dim3(blocks), dim3(ENVS_PER_BLOCK * WAVE), 0, s,
                       *p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int hwy_launch_lookahead_choice(const LookaheadParams* p, hipStream_t s) {
  const int blocks = (p->p.cfg.num_envs + 255) / 256;
  hipLaunchKernelGGL(hwy_lookahead_choice_kernel, dim3(blocks), dim3(256), 0, s, *p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#elif defined(HWY_GRID_TU)
// hwy_grid's kernel, likewise a unit of its own (-DHWY_GRID_TU -> hwy_grid.o): the occupancy grid
// of include/hwy.h.  One wave per env, lane = vehicle, as the step; it loads the five fields the
// observation reads (x, y, heading, speed, flags), 1,280 B per env, and writes nothing but the
// outputs it was given.  The owner of every cell lives in per-wave LDS (nx * ny words, dynamic):
// filled with the sentinel WAVE, then taken with an LDS integer minimum on the vehicle index.
// Each lane lays its own per-layer values out in lds_val; an output element reads its value
// through its cell's owner, and consecutive lanes store consecutive floats of the row.  Every
// cross-lane read runs with all 64 lanes active; an LDS index is the lane, a bounded loop index
// or a cell index that passed the inside test.
__global__ void __launch_bounds__(256) hwy_grid_kernel(GridParams P) {
  extern __shared__ int lds_own_all[];  // [ENVS_PER_BLOCK][nx * ny]
  __shared__ float lds_val[ENVS_PER_BLOCK][HWY_GRID_MAX_LAYERS][WAVE];
  __shared__ float lds_tail[ENVS_PER_BLOCK][HWY_MAX_FEATURES];
  const hwy_config& C = P.cfg;
  const hwy_grid_args& A = P.a;
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = threadIdx.x / WAVE;
  const int e = blockIdx.x * ENVS_PER_BLOCK + w;
  if (e >= C.num_envs) return;  // whole wave
  const int V = C.vehicles_count + 1;
  const int F = C.n_features;
  const int ncells = A.nx * A.ny;  // <= HWY_GRID_MAX_CELLS
  int* own = lds_own_all + w * ncells;
  const size_t fstride = (size_t)C.num_envs * WAVE;
  const uint32_t idx = (uint32_t)e * WAVE + lane;  // < 2^32: hwy_create bounds num_envs
  const uint32_t* st = P.state;
  const float x = hm_bits2f((st + HWY_F_X * fstride)[idx]);
  const float y = hm_bits2f((st + HWY_F_Y * fstride)[idx]);
  const float h = hm_bits2f((st + HWY_F_HEADING * fstride)[idx]);
  const float spd = hm_bits2f((st + HWY_F_SPEED * fstride)[idx]);
  const uint32_t fl = (st + HWY_F_FLAGS * fstride)[idx];
  const bool present = ((fl & HWY_FLAG_PRESENT) != 0u) && lane < V;  // load_veh's rule
  float cos_h, sin_h;
  hm_sincosf(h, &sin_h, &cos_h);
  const float ex = rdlf(x, 0), ey = rdlf(y, 0), eh = rdlf(h, 0), espd = rdlf(spd, 0);
  const float ec = rdlf(cos_h, 0), es = rdlf(sin_h, 0);

  // ---- the cell of this lane's vehicle
  const float dx = x - ex, dy = y - ey;
  float u = dx, ww = dy;
  if (A.align) {
    u = dx * ec + dy * es;
    ww = dy * ec - dx * es;
  }
  const float qx = (u - A.x0) / A.step_x, qy = (ww - A.y0) / A.step_y;
  // in float, before any conversion: a NaN or an infinity fails a comparison and is never an index
  const bool inside =
      present && qx >= 0.0f && qx < (float)A.nx && qy >= 0.0f && qy < (float)A.ny;
  int cell = 0;
  if (inside) cell = (int)hm_floorf(qx) * A.ny + (int)hm_floorf(qy);  // in 0..ncells-1

  // ---- the owners: the least inside vehicle index per cell
  for (int c = lane; c < ncells; c += WAVE) own[c] = WAVE;
  wave_lds_sync();
  if (inside) atomicMin(&own[cell], lane);

  // ---- this vehicle's value per layer, and the ego tail (lane f holds feature f)
#pragma unroll
  for (int l = 0; l < HWY_GRID_MAX_LAYERS; ++l)
    if (l < A.n_layers) {
      const int fid = A.layer_ids[l];
      float val = 0.0f;  // the on_road layer reads nothing from here
      if (fid != HWY_GRID_ON_ROAD) {
        val = feature_value(fid, x, y, spd, h, cos_h, sin_h);
        if (is_relative_feature(fid)) val = val - feature_value(fid, ex, ey, espd, eh, ec, es);
        if (A.has_range[l]) {
          val = hm_lmap(val, A.range[l][0], A.range[l][1], -1.0f, 1.0f);
          if (A.clip) val = hm_clipf(val, -1.0f, 1.0f);
        }
      }
      lds_val[w][l][lane] = val;
    }
  float tv = 0.0f;
  if (A.ego_tail) {
#pragma unroll
    for (int f = 0; f < HWY_MAX_FEATURES; ++f)
      if (f < F) {
        float val = feature_value(C.feature_ids[f], ex, ey, espd, eh, ec, es);
        if (C.normalize && C.has_range[f]) {
          val = hm_lmap(val, C.features_range[f][0], C.features_range[f][1], -1.0f, 1.0f);
          if (C.clip) val = hm_clipf(val, -1.0f, 1.0f);
        }
        tv = lane == f ? val : tv;
      }
  }
  if (lane < HWY_MAX_FEATURES) lds_tail[w][lane] = tv;
  wave_lds_sync();

  // ---- the row: the layers, the ego tail, the padding
  if (A.grid) {
    float* row = A.grid + (size_t)e * A.row_stride;
#pragma unroll
    for (int l = 0; l < HWY_GRID_MAX_LAYERS; ++l)
      if (l < A.n_layers) {
        float* lay = row + l * ncells;
        if (A.layer_ids[l] == HWY_GRID_ON_ROAD) {
          const float y_hi = (float)(4 * C.lanes_count - 2);
          for (int c = lane; c < ncells; c += WAVE) {
            const int i = c / A.ny, j = c - i * A.ny;
            const float gx = A.x0 + ((float)i + 0.5f) * A.step_x;
            const float gy = A.y0 + ((float)j + 0.5f) * A.step_y;
            float rx = gx, ry = gy;
            if (A.align) {
              rx = gx * ec - gy * es;
              ry = gx * es + gy * ec;
            }
            const float X = ex + rx, Y = ey + ry;
            const bool on = 0.0f <= X && X <= ROAD_LENGTH && -2.0f <= Y && Y < y_hi;
            lay[c] = on ? 1.0f : 0.0f;
          }
        } else {
          for (int c = lane; c < ncells; c += WAVE) {
            const int o = own[c];
            const float val = lds_val[w][l][o < WAVE ? o : 0];
            lay[c] = o < WAVE ? val : 0.0f;
          }
        }
      }
    const int base = A.n_layers * ncells;
    for (int k = base + lane; k < A.row_stride; k += WAVE) {
      const int f = k - base;
      const float val = lds_tail[w][f < HWY_MAX_FEATURES ? f : 0];
      row[k] = (A.ego_tail && f < F) ? val : 0.0f;
    }
  }
  if (A.cell_vehicle)
    for (int c = lane; c < ncells; c += WAVE) {
      const int o = own[c];
      A.cell_vehicle[(size_t)e * ncells + c] = o < WAVE ? o : -1;
    }
  if (A.veh_cell) A.veh_cell[idx] = inside ? cell : -1;
  if (A.counts) {
    const bool other = present && lane >= 1;
    bool lost = false;
    if (inside) lost = own[cell] != lane;
    const uint64_t otherm = ballot(other);
    const uint64_t inm = ballot(other && inside);
    const uint64_t lostm = ballot(other && lost);
    int cv = __popcll(otherm);
    cv = lane == 1 ? __popcll(inm) : cv;
    cv = lane == 2 ? __popcll(lostm) : cv;
    cv = lane == 3 ? __popcll(otherm & ~inm) : cv;
    if (lane < 4) A.counts[(size_t)e * 4 + lane] = cv;
  }
}

extern "C" int hwy_launch_grid(const GridParams* p, hipStream_t s) {
  const int blocks = (p->cfg.num_envs + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  const size_t lds = (size_t)ENVS_PER_BLOCK * p->a.nx * p->a.ny * sizeof(int);
  hipLaunchKernelGGL(hwy_grid_kernel, dim3(blocks), dim3(ENVS_PER_BLOCK * WAVE), lds, s, *p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#elif defined(HWY_LIDAR_TU)
// hwy_lidar's kernel, likewise a unit of its own (-DHWY_LIDAR_TU -> hwy_lidar.o): the ray-cast
// range observation of include/hwy.h.  One wave per env.  Lanes first act as vehicles: each loads
// the five fields the rule reads and the env words (1,536 B per env), runs hm_sincosf once and
// lays the ego's centre in its own frame (ou, ow), its axes and its velocity out in per-wave LDS.
// Lanes then act as cells, strided by 64: a cell runs its sub-rays one after the other, each over
// the present bodies in ascending index with broadcast LDS reads, and keeps the first strict
// minimum, which is the rule's tie order (least j, then least k).  The cell loop's trip count is
// wave-uniform, so every ballot and every LDS-synchronised step runs with all 64 lanes active; an
// LDS index is the lane, a bounded loop index (k < V <= 64) or the winner such a loop left.
// `seen` comes from per-wave LDS flags, the counts from ballots.

// one Philox draw of a cell's stream: counter (cell, step word, channel, salt word)
__device__ __forceinline__ hm_u32x4 lidar_draw(int cell, int step, uint32_t ch, uint32_t salt_word,
                                               uint64_t seed) {
  return hm_philox4x32_10((uint32_t)cell, (uint32_t)step, ch, salt_word,
                          (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
}

// one axis of the slab test: false for an empty interval, else its ends
__device__ __forceinline__ bool lidar_axis(float o, float d, float H, float* lo, float* hi) {
  if (d == 0.0f) {
    *lo = -__builtin_inff();
    *hi = __builtin_inff();
    return hm_absf(o) <= H;
  }
  const float t1 = (-H - o) / d, t2 = (H - o) / d;
  *lo = hm_minf(t1, t2);
  *hi = hm_maxf(t1, t2);
  return true;
}

__global__ void __launch_bounds__(256) hwy_lidar_kernel(LidarParams P) {
  __shared__ float4 lds_body[ENVS_PER_BLOCK][WAVE];  // (ou, ow, cos h, sin h)
  __shared__ float2 lds_vel[ENVS_PER_BLOCK][WAVE];   // (vx, vy)
  __shared__ int lds_seen[ENVS_PER_BLOCK][WAVE];
  __shared__ float lds_tail[ENVS_PER_BLOCK][HWY_MAX_FEATURES];
  const hwy_config& C = P.cfg;
  const hwy_lidar_args& A = P.a;
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = threadIdx.x / WAVE;
  const int e = blockIdx.x * ENVS_PER_BLOCK + w;
  if (e >= C.num_envs) return;  // whole wave
  const int V = C.vehicles_count + 1;
  const int F = C.n_features;
  const size_t fstride = (size_t)C.num_envs * WAVE;
  const uint32_t idx = (uint32_t)e * WAVE + lane;  // < 2^32: hwy_create bounds num_envs
  const uint32_t* st = P.state;
  const float x = hm_bits2f((st + HWY_F_X * fstride)[idx]);
  const float y = hm_bits2f((st + HWY_F_Y * fstride)[idx]);
  const float h = hm_bits2f((st + HWY_F_HEADING * fstride)[idx]);
  const float spd = hm_bits2f((st + HWY_F_SPEED * fstride)[idx]);
  const uint32_t fl = (st + HWY_F_FLAGS * fstride)[idx];
  const uint32_t ew = (st + HWY_F_ENV * fstride)[idx];
  const bool present = ((fl & HWY_FLAG_PRESENT) != 0u) && lane < V;  // load_veh's rule
  const int step = rdli((int)ew, HWY_E_STEP);
  const uint64_t seed = (uint64_t)(uint32_t)rdli((int)ew, HWY_E_SEED_LO) |
                        ((uint64_t)(uint32_t)rdli((int)ew, HWY_E_SEED_HI) << 32);
  float cos_h, sin_h;
  hm_sincosf(h, &sin_h, &cos_h);
  const float ex = rdlf(x, 0), ey = rdlf(y, 0), eh = rdlf(h, 0), espd = rdlf(spd, 0);
  const float ec = rdlf(cos_h, 0), es = rdlf(sin_h, 0);

  // ---- lanes as vehicles: the ego's centre in this body's frame, its axes, its velocity
  const float ox = ex - x, oy = ey - y;
  const float vx = spd * cos_h, vy = spd * sin_h;
  const float evx = rdlf(vx, 0), evy = rdlf(vy, 0);
  lds_body[w][lane] = make_float4(ox * cos_h + oy * sin_h, oy * cos_h - ox * sin_h, cos_h, sin_h);
  lds_vel[w][lane] = make_float2(vx, vy);
  lds_seen[w][lane] = 0;
  float tv = 0.0f;  // the ego tail: lane f holds feature f, as in the grid
  if (A.ego_tail) {
#pragma unroll
    for (int f = 0; f < HWY_MAX_FEATURES; ++f)
      if (f < F) {
        float val = feature_value(C.feature_ids[f], ex, ey, espd, eh, ec, es);
        if (C.normalize && C.has_range[f]) {
          val = hm_lmap(val, C.features_range[f][0], C.features_range[f][1], -1.0f, 1.0f);
          if (C.clip) val = hm_clipf(val, -1.0f, 1.0f);
        }
        tv = lane == f ? val : tv;
      }
  }
  if (lane < HWY_MAX_FEATURES) lds_tail[w][lane] = tv;
  const uint64_t otherm = ballot(present && lane >= 1);
  // Only a hit with d <= range_m counts.  A body whose centre is more than (range_m + 4 m) *
  // 1.0001 from the ego (its half diagonal is 2.7 m) has no point within a metre of that range,
  // so no ray can count a hit on it and it is left out of the loop: wave-uniformly, and never on
  // a NaN distance (the comparison is false).  The same cull, with the same margins, as hwy_sense.
  const uint64_t bodym = otherm & ~ballot(ox * ox + oy * oy > P.cull2);
  wave_lds_sync();

  // ---- lanes as cells
  const float off = 0.5f - 0.5f * (float)A.sub;
  float* row = A.obs ? A.obs + (size_t)e * A.row_stride : nullptr;
  int nret = 0, ndrop = 0;  // wave-uniform
  for (int c0 = 0; c0 < A.cells; c0 += WAVE) {
    const int c = c0 + lane;
    const bool live = c < A.cells;
    float best = __builtin_inff(), bdx = 0.0f, bdy = 0.0f;
    int bk = -1;
    if (live) {
      for (int j = 0; j < A.sub; ++j) {
        float theta = ((float)(c * A.sub + j) + off) * P.dth;
        if (A.align) theta = theta + eh;
        float dx, dy;
        hm_sincosf(theta, &dy, &dx);
        for (int k = 1; k < V; ++k) {
          if (!((bodym >> k) & 1ull)) continue;  // wave-uniform: absent, or out of reach
          const float4 b = lds_body[w][k];
          const float du = dx * b.z + dy * b.w;
          const float dw = dy * b.z - dx * b.w;
          float lo_u, hi_u, lo_w, hi_w;
          const bool ok_u = lidar_axis(b.x, du, 0.5f * VEH_LENGTH, &lo_u, &hi_u);
          const bool ok_w = lidar_axis(b.y, dw, 0.5f * VEH_WIDTH, &lo_w, &hi_w);
          const float t_in = hm_maxf(lo_u, lo_w), t_out = hm_minf(hi_u, hi_w);
          const float d = t_in > 0.0f ? t_in : 0.0f;
          const bool counted = ok_u && ok_w && t_in <= t_out && t_out >= 0.0f && d <= A.range_m;
          if (counted && d < best) {  // strict: the first of equal distances stays
            best = d;
            bk = k;
            bdx = dx;
            bdy = dy;
          }
        }
      }
    }
    bool dropped = false;
    if (A.p_drop > 0.0f)  // u < 0 never holds
      dropped = hm_u01(lidar_draw(c, step, 0u, P.salt_word, seed).v[0]) < A.p_drop;
    const bool ret = live && bk >= 0 && !dropped;
    float dist = A.range_m, vel = 0.0f;
    if (ret) {
      const float2 vk = lds_vel[w][bk];  // bk: 1..V-1
      dist = best;
      vel = ((vk.x - evx) * bdx) + ((vk.y - evy) * bdy);
    }
    if (A.sigma_r != 0.0f) {  // a sigma of exactly 0 skips the addition
      const hm_u32x4 r = lidar_draw(c, step, 1u, P.salt_word, seed);
      const float u0 = hm_u01(r.v[0]), u1 = hm_u01(r.v[1]), u2 = hm_u01(r.v[2]), u3 = hm_u01(r.v[3]);
      const float z = (((u0 + u1) + (u2 + u3)) - 2.0f) * 1.7320508f;
      if (ret) dist = hm_clipf(dist + A.sigma_r * z, 0.0f, A.range_m);
    }
    if (A.normalize) {
      dist = dist / A.range_m;
      vel = vel / A.speed_scale;
    }
    if (live) {
      if (row) {
        row[2 * c] = dist;
        row[2 * c + 1] = vel;
      }
      if (A.hit_vehicle) A.hit_vehicle[(size_t)e * A.cells + c] = ret ? bk : -1;
    }
    if (ret) lds_seen[w][bk] = 1;
    nret += __popcll(ballot(ret));
    ndrop += __popcll(ballot(live && dropped));
  }
  wave_lds_sync();

  // ---- the ego tail and the padding; seen; counts
  if (row) {
    const int base = 2 * A.cells;
    for (int k = base + lane; k < A.row_stride; k += WAVE) {
      const int f = k - base;
      const float val = lds_tail[w][f < HWY_MAX_FEATURES ? f : 0];
      row[k] = (A.ego_tail && f < F) ? val : 0.0f;
    }
  }
  const bool sv = lds_seen[w][lane] != 0;
  if (A.seen) A.seen[idx] = sv ? 1.0f : 0.0f;
  if (A.counts) {
    const uint64_t seenm = ballot(sv);  // all 64 lanes: not inside the select below
    int cv = __popcll(otherm);
    cv = lane == 1 ? __popcll(seenm) : cv;
    cv = lane == 2 ? nret : cv;
    cv = lane == 3 ? ndrop : cv;
    if (lane < 4) A.counts[(size_t)e * 4 + lane] = cv;
  }
}

extern "C" int hwy_launch_lidar(const LidarParams* p, hipStream_t s) {
  const int blocks = (p->cfg.num_envs + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  hipLaunchKernelGGL(hwy_lidar_kernel, dim3(blocks), dim3(ENVS_PER_BLOCK * WAVE), 0, s, *p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#else  // the main unit, to the end of the file
template <int W>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, 8)))
hwy_step_kernel(StepParams P) {
  step_body<W, false>(P, nullptr);
}

// handle blockIdx.y of tab; blocks past a handle's envs exit in step_body (whole waves).  The
// profiling builds' per-env clocks and section counters index by env within the handle.
template <int W>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, 8)))
hwy_step_grp_kernel(const StepParams* __restrict__ tab) {
  step_body<W, false>(tab[blockIdx.y], nullptr);
}

__global__ void __launch_bounds__(256) hwy_reset_kernel(StepParams P) {
  __shared__ int lds_vor[ENVS_PER_BLOCK][WAVE];
  __shared__ int lds_inv[ENVS_PER_BLOCK][WAVE];
  __shared__ unsigned long long lds_key[ENVS_PER_BLOCK][WAVE];
  const hwy_config& C = P.cfg;
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = threadIdx.x / WAVE;
  const int e = blockIdx.x * ENVS_PER_BLOCK + w;
  if (e >= C.num_envs) return;
  if (P.mask && !P.mask[e]) return;
  const int V = C.vehicles_count + 1;
  const size_t fstride = (size_t)C.num_envs * WAVE;
  const uint32_t idx = (uint32_t)e * WAVE + lane;  // < 2^32: hwy_create bounds num_envs
  const uint64_t seed = P.seeds ? P.seeds[e] : episode_seed(P, e, 0);
  Veh v;
  reset_wave(C, lane, seed, v);
  if (P.obs)
    observe_wave(C, lane, v, 1.0f, 0.0f, 0, seed, group_pe_table(P, e),
                 P.obs + (size_t)e * C.obs_vehicles * P.fout, P.fout, lds_vor[w], lds_inv[w],
                 lds_key[w]);
  store_veh(P.state, fstride, idx, lane, V, v, reset_order_pos(lane, V));
  store_env_words(P.state, fstride, idx, lane, 0, 0, seed, 0.0f, 0.0f, 0.0f);
}

// Stand-alone wrapper on [E,N,F]: one thread per (env, row).
__global__ void __launch_bounds__(256) hwy_obs_pe_kernel(const float* __restrict__ in,
                                                         float* __restrict__ out, int E, int N,
                                                         int F, int kind, int d, int ego_idx,
                                                         float max_dist, const float* table,
                                                         const float* dist_override) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)E * N) return;
  const long e = t / N;
  const int r = (int)(t - e * N);
  const int Fo = F + ((kind == HWY_PE_RANK || kind == HWY_PE_DIST || kind == HWY_PE_DIST1) ? d : 0);
  float vals[HWY_MAX_FEATURES];
#pragma unroll
  for (int f = 0; f < HWY_MAX_FEATURES; ++f) vals[f] = f < F ? in[t * F + f] : 0.0f;
  const float* eg = in + (e * N + ego_idx) * F;
  const float ex0 = eg[0], ex1 = F > 1 ? eg[1] : 0.0f;
  write_pe_row(vals, F, kind, d, r, ex0, ex1, max_dist, table, dist_override != nullptr,
               dist_override ? dist_override[t] : 0.0f, out + t * Fo);
}

// PPOMemory.compute_advantages on [T,E]: one thread per env, reversed scan over t.
__global__ void __launch_bounds__(64) hwy_gae_kernel(const float* __restrict__ rew,
                                                      const uint8_t* __restrict__ done,
                                                      const float* __restrict__ val,
                                                      const float* __restrict__ last_val,
                                                      double gamma, double lam, int T, int E,
                                                      float* __restrict__ adv,
                                                      float* __restrict__ ret) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const double gl = gamma * lam;
  float last_adv = 0.0f;
  double v1 = (double)last_val[e];
  // the recurrence is sequential per env (each step rounds to float, as the reference's float
  // tensors do), but its inputs are not: kGaeAhead steps' rewards, values and dones are loaded
  // before they are used, so one memory round trip serves kGaeAhead steps instead of one
  constexpr int kGaeAhead = 8;
  for (int t1 = T; t1 > 0; t1 -= kGaeAhead) {
    float rv[kGaeAhead], vv[kGaeAhead];
    uint8_t dv[kGaeAhead];
#pragma unroll
    for (int j = 0; j < kGaeAhead; ++j) {
      const int t = t1 - 1 - j;
      const size_t i = (size_t)(t < 0 ? 0 : t) * E + e;
      rv[j] = rew[i], vv[j] = val[i], dv[j] = done[i];
    }
#pragma unroll
    for (int j = 0; j < kGaeAhead; ++j) {
      const int t = t1 - 1 - j;
      if (t < 0) break;
      const size_t i = (size_t)t * E + e;
      const float v0f = vv[j];
      const double nd = dv[j] ? 0.0 : 1.0;
      const double delta = ((double)rv[j] + (gamma * v1) * nd) - (double)v0f;
      const float a = (float)(delta + (gl * nd) * (double)last_adv);
      adv[i] = a;
      ret[i] = a + v0f;
      last_adv = a;
      v1 = (double)v0f;
    }
  }
}

__global__ void hwy_math_kernel(int op, const float* in, const float* in2, float* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = in[i], y = in2 ? in2[i] : 0.0f;
  float r = 0.0f;
  switch (op) {
    case 0: r = hm_sinf(x); break;
    case 1: r = hm_cosf(x); break;
    case 2: r = hm_tanf(x); break;
    case 3: r = hm_atanf(x); break;
    case 4: r = hm_asinf(x); break;
    case 5: r = hm_expf(x); break;
    case 6: r = hm_logf(x); break;
    case 7: r = hm_powf(x, y); break;
    case 8: r = hm_wrap_to_pi(x); break;
    case 9: r = __builtin_sqrtf(x); break;
    case 10: r = x / y; break;
    case 11: r = hm_floorf(x); break;
    case 12: { float c_; hm_sincosf(x, &r, &c_); } break;
    case 13: { float s_; hm_sincosf(x, &s_, &r); } break;
    case 14: r = hm_tanf_sc(x); break;
    case 15: r = hm_powf_idm(x, y); break;
    case 16: r = (float)closest_lane(x, (int)y); break;  // y: lanes_count
  }
  out[i] = r;
}

// ------------------------------------------------------------------------- launch helpers
extern "C" {
// compute units of the current device (cached per device; 256 without one)
// envs per CU above which the big build runs: at 8,192 envs (32 per CU) the 4-wave build is
// 6-7 % faster than the 6-wave one (0.205 vs 0.219-0.245 ms per step), at 16,384 the 6-wave build
// wins (0.295 vs 0.324) and at 32,768 ties the 5-wave one (profiles/r6/micro/ab_bigw.log)
#ifndef HWY_STEP_BIG_WAVES
#define HWY_STEP_BIG_WAVES 32
#endif
constexpr int kStepBigW = HWY_STEP_BIG_W;
static int device_cus() {
  static int cache[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    (void)hipGetLastError();
    return 256;
  }
  if (!cache[dev]) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus < 1)
      cus = 256;
    (void)hipGetLastError();
    cache[dev] = cus;
  }
  return cache[dev];
}

int hwy_launch_step(const StepParams* p, hipStream_t s) {
  const int blocks = (p->cfg.num_envs + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  // one wave per env: more than 4 waves per SIMD of envs queue behind the first four
  if (hwy_step_big(p->cfg.num_envs))
    hipLaunchKernelGGL(hwy_step_kernel<kStepBigW>, dim3(blocks), dim3(ENVS_PER_BLOCK * WAVE), 0, s, *p);
  else
    hipLaunchKernelGGL(hwy_step_kernel<4>, dim3(blocks), dim3(ENVS_PER_BLOCK * WAVE), 0, s, *p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int hwy_launch_step_group(const StepParams* dtab, int n, int blocks, int big, hipStream_t s) {
  if (big)
    hipLaunchKernelGGL(hwy_step_grp_kernel<kStepBigW>, dim3(blocks, n), dim3(ENVS_PER_BLOCK * WAVE),
                       0, s, dtab);
  else
    hipLaunchKernelGGL(hwy_step_grp_kernel<4>, dim3(blocks, n), dim3(ENVS_PER_BLOCK * WAVE), 0, s,
                       dtab);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int hwy_step_blocks(int num_envs) { return (num_envs + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK; }
int hwy_step_big(int64_t total_envs) {
  return total_envs > (int64_t)HWY_STEP_BIG_WAVES * device_cus() ? 1 : 0;
}
int hwy_launch_reset(const StepParams* p, hipStream_t s) {
  const int blocks = (p->cfg.num_envs + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  hipLaunchKernelGGL(hwy_reset_kernel, dim3(blocks), dim3(ENVS_PER_BLOCK * WAVE), 0, s, *p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int hwy_launch_obs_pe(const float* in, float* out, int E, int N, int F, int kind, int d, int ego,
                      float max_dist, const float* table, const float* dov, hipStream_t s) {
  const long n = (long)E * N;
  if (n == 0) return 0;
  const int blocks = (int)((n + 255) / 256);
  hipLaunchKernelGGL(hwy_obs_pe_kernel, dim3(blocks), dim3(256), 0, s, in, out, E, N, F, kind, d,
                     ego, max_dist, table, dov);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int hwy_launch_gae(const float* rew, const uint8_t* done, const float* val, const float* last_val,
                   double gamma, double lam, int T, int E, float* adv, float* ret, hipStream_t s) {
  if (E == 0) return 0;
  // one wave per workgroup: 4,096 envs spread over 64 CUs instead of 16
  const int blocks = (E + 63) / 64;
  hipLaunchKernelGGL(hwy_gae_kernel, dim3(blocks), dim3(64), 0, s, rew, done, val, last_val,
                     gamma, lam, T, E, adv, ret);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int hwy_launch_math(int op, const float* in, const float* in2, float* out, int n, hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(hwy_math_kernel, dim3((n + 255) / 256), dim3(256), 0, s, op, in, in2, out, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
}

#if defined(HWY_SECTION_PROFILE) || defined(HWY_WAVE_TIMES)
extern "C" int hwy_debug_wave_times(unsigned long long* out, int n) {
  if (n > 5 * HWY_NWT) n = 5 * HWY_NWT;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hwy_wave_t), sizeof(unsigned long long) * n) ==
                 hipSuccess ? 0 : -2;
}
#endif
#ifdef HWY_SECTION_PROFILE
// development build only: copy out (and optionally clear) the section clock totals
// development build only: the per-env totals themselves ([n][HWY_NSEC], n <= HWY_NSEC_ENVS)
extern "C" int hwy_debug_sections_env(unsigned long long* out, int n) {
  if (!out || n < 0) return -1;
  if (n > HWY_NSEC_ENVS) n = HWY_NSEC_ENVS;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hwy_sections),
                             sizeof(unsigned long long) * HWY_NSEC * n) == hipSuccess ? 0 : -2;
}
extern "C" int hwy_debug_sections(unsigned long long* out, int reset) {
  static unsigned long long h[HWY_NSEC_ENVS][HWY_NSEC];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_hwy_sections), sizeof(h)) != hipSuccess) return -2;
  for (int i = 0; i < HWY_NSEC; ++i) out[i] = 0;
  for (int e = 0; e < HWY_NSEC_ENVS; ++e)
    for (int i = 0; i < HWY_NSEC; ++i) out[i] += h[e][i];
  if (reset) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_hwy_sections)) != hipSuccess) return -2;
    if (hipMemset(p, 0, sizeof(h)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -2;
  }
  return 0;
}
#endif
#endif  // HWY_CUT_TU / HWY_INFO_TU / HWY_FINAL_TU / HWY_OBSERVE_TU / HWY_TRAFFIC_TU / HWY_SENSE_TU /
        // HWY_LOOKAHEAD_TU / HWY_GRID_TU / HWY_LIDAR_TU
