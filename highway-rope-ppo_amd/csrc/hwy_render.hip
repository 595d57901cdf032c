// hwy_render.hip -- hwy_render's rasteriser: env states -> uint8 frames by the frame rule of
// include/hwy.h.  A unit of its own, so no other object's code changes with it.
//
// One workgroup of 256 threads draws 4,096 consecutive pixels of one frame (a band of rows; the
// pixels of a frame are taken in memory order, so a band may begin and end inside a row).  Wave 0
// first loads the env's 64 vehicles, one lane each, forms the ego-relative centres and sin / cos,
// drops the vehicles that cannot reach the band -- the view's x extent and the band's rows, grown
// by kCull -- and compacts the rest by ballot into LDS in painter's order (ascending index, the
// ego last).  Every thread then owns 16 consecutive pixels: it walks the survivor list once
// (wave-uniform LDS reads), keeping the 16 colours in registers, and writes them as one 16-byte
// store (luma) or three (RGB).  A frame's first byte is 16-byte aligned whenever the frame's byte
// length is a multiple of 16 (600x150x3 and 64x128x1 are); a frame that starts off that
// alignment, and the last partial group of a frame, are written with byte stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hwy.h"
#include "hwy_internal.h"
#include "hwy_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kGroup = 16;                       // pixels per thread
constexpr int kBlockPixels = kThreads * kGroup;  // pixels per workgroup

constexpr uint32_t rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }
constexpr uint32_t kBackground = rgb(60, 60, 60);
constexpr uint32_t kRoad = rgb(100, 100, 100);
constexpr uint32_t kLine = rgb(255, 255, 255);
constexpr uint32_t kVehicle = rgb(100, 200, 255);
constexpr uint32_t kEgo = rgb(50, 200, 0);
constexpr uint32_t kCrashed = rgb(255, 100, 100);
constexpr uint32_t kHot = rgb(255, 220, 0);
constexpr float kLineHalf = 0.15f;
constexpr float kDashOn = 3.0f, kDashPeriod = 8.0f;
constexpr float kHalfLength = 2.5f, kHalfWidth = 1.0f;  // VEH_LENGTH / 2, VEH_WIDTH / 2
constexpr float kRoadLength = 10000.0f;
// a covered pixel lies within the half-diagonal sqrt(2.5^2 + 1^2) = 2.6926 m of the vehicle's
// centre; rounded up so that no binary32 rounding of the test's operands can cull a covered pixel
constexpr float kCull = 2.7f;

__device__ inline uint32_t luma_of(uint32_t c) {
  return (77u * (c & 255u) + 150u * ((c >> 8) & 255u) + 29u * ((c >> 16) & 255u) + 128u) >> 8;
}

__device__ inline uint32_t tint(uint32_t base, float s) {
  const float t = (s > 0.0f) ? (s < 1.0f ? s : 1.0f) : 0.0f;  // NaN -> 0
  const uint32_t s8 = (uint32_t)(int)(t * 256.0f);
  uint32_t out = 0;
  for (int k = 0; k < 24; k += 8) {
    const uint32_t b = (base >> k) & 255u, h = (kHot >> k) & 255u;
    out |= ((b * (256u - s8) + h * s8 + 128u) >> 8) << k;
  }
  return out;
}

// what one row of the frame contributes to its pixels' first three layers
struct Row {
  float py;
  bool surface;  // y_0 <= py < y_L
  int line;      // 0 none, 1 solid, 2 dashed
};

__device__ inline Row row_of(int r, float ch_h, float scaling, float ye, int lanes) {
  Row o;
  o.py = (((float)r + 0.5f) - ch_h) / scaling;
  const float y0 = -2.0f - ye, yl = (float)(4 * lanes - 2) - ye;
  o.surface = y0 <= o.py && o.py < yl;
  // lines are 4 m apart: only the nearest one can be within kLineHalf
  const float t = (o.py + ye + 2.0f) * 0.25f;
  o.line = 0;
  if (t > -1.0f && t < (float)(lanes + 1)) {
    int k = (int)hm_floorf(t + 0.5f);
    k = k < 0 ? 0 : (k > lanes ? lanes : k);
    const float yk = (float)(4 * k - 2) - ye;
    if (hm_absf(o.py - yk) <= kLineHalf) o.line = (k == 0 || k == lanes) ? 1 : 2;
  }
  return o;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void hwy_render_kernel(const RenderParams p) {
  __shared__ float s_cx[HWY_MAX_VEHICLES], s_cy[HWY_MAX_VEHICLES];
  __shared__ float s_ch[HWY_MAX_VEHICLES], s_sh[HWY_MAX_VEHICLES];
  __shared__ uint32_t s_col[HWY_MAX_VEHICLES];
  __shared__ float s_ego[3];  // xe, ye, dash phase
  __shared__ int s_n;

  const int frame = (int)blockIdx.x;
  const int W = p.a.width, H = p.a.height, C = p.a.channels;
  const int HW = W * H;  // <= 2^24
  const int p0 = (int)blockIdx.y * kBlockPixels;
  const float scaling = p.a.scaling;
  const float cw_w = p.a.centering[0] * (float)W, ch_h = p.a.centering[1] * (float)H;
  const bool luma = C == 1;

  if (threadIdx.x < HWY_MAX_VEHICLES) {  // wave 0, lane v = vehicle v
    const int v = (int)threadIdx.x;
    const int e = p.a.env_ids ? p.a.env_ids[frame] : frame;
    const bool valid = e >= 0 && e < p.num_envs;  // else: never index with it, all background
    float x = hm_bits2f(0x7fc00000u), y = x, heading = 0.0f, shade = 0.0f;
    uint32_t flags = 0;
    if (valid) {
      const size_t E = (size_t)p.num_envs;
      const size_t at = (size_t)e * HWY_MAX_VEHICLES + (size_t)v;
      x = hm_bits2f(p.state[(HWY_F_X * E) * HWY_MAX_VEHICLES + at]);
      y = hm_bits2f(p.state[(HWY_F_Y * E) * HWY_MAX_VEHICLES + at]);
      heading = hm_bits2f(p.state[(HWY_F_HEADING * E) * HWY_MAX_VEHICLES + at]);
      flags = p.state[(HWY_F_FLAGS * E) * HWY_MAX_VEHICLES + at];
      if (p.a.shade) shade = p.a.shade[at];
    }
    const float xe = __shfl(x, 0), ye = __shfl(y, 0);
    const float cx = x - xe, cy = y - ye;
    float sh, ch;
    hm_sincosf(heading, &sh, &ch);
    // the band's rectangle in metres from the ego, grown by kCull
    const int last = (p0 + kBlockPixels < HW ? p0 + kBlockPixels : HW) - 1;
    const float xlo = (0.5f - cw_w) / scaling - kCull;
    const float xhi = (((float)(W - 1) + 0.5f) - cw_w) / scaling + kCull;
    const float ylo = (((float)(p0 / W) + 0.5f) - ch_h) / scaling - kCull;
    const float yhi = (((float)(last / W) + 0.5f) - ch_h) / scaling + kCull;
    const bool reach = cx >= xlo && cx <= xhi && cy >= ylo && cy <= yhi;
    // the distance bound holds for a unit (ch, sh) only: hm_sincosf gives (0, 0) past 2^24,
    // where the coverage test is true wherever it is finite; such a vehicle is never culled
    const bool degenerate = ch * ch + sh * sh <= 0.5f;
    const bool keep = valid && (v == 0 || (flags & HWY_FLAG_PRESENT)) && (reach || degenerate);
    const unsigned long long others = __ballot(keep && v != 0);
    const int n_others = __popcll(others);
    const int pos = v == 0 ? n_others : __popcll(others & ((1ull << v) - 1ull));
    if (keep) {
      uint32_t col = (flags & HWY_FLAG_CRASHED) ? kCrashed : (v == 0 ? kEgo : kVehicle);
      col = tint(col, shade);
      s_cx[pos] = cx;
      s_cy[pos] = cy;
      s_ch[pos] = ch;
      s_sh[pos] = sh;
      s_col[pos] = luma ? luma_of(col) : col;
    }
    if (v == 0) {
      s_n = n_others + (keep ? 1 : 0);
      s_ego[0] = xe;
      s_ego[1] = ye;
      s_ego[2] = xe - kDashPeriod * hm_floorf(xe / kDashPeriod);
    }
  }
  __syncthreads();

  const int pix = p0 + (int)threadIdx.x * kGroup;
  if (pix >= HW) return;
  const int n = s_n;
  const float xe = s_ego[0], ye = s_ego[1], phase = s_ego[2];
  const float road_lo = -xe, road_hi = kRoadLength - xe;
  const uint32_t c_bg = luma ? luma_of(kBackground) : kBackground;
  const uint32_t c_road = luma ? luma_of(kRoad) : kRoad;
  const uint32_t c_line = luma ? luma_of(kLine) : kLine;

  // layers 1-3 of the thread's 16 pixels (those past the frame's end are computed and dropped)
  float px[kGroup], py[kGroup];
  uint32_t col[kGroup];
  int r = pix / W, c = pix - r * W;
  Row row = row_of(r, ch_h, scaling, ye, p.lanes_count);
#pragma unroll
  for (int j = 0; j < kGroup; ++j) {
    const float x = (((float)c + 0.5f) - cw_w) / scaling;
    px[j] = x;
    py[j] = row.py;
    const bool in_x = road_lo <= x && x <= road_hi;
    bool on_line = row.line == 1;
    if (row.line == 2) {
      const float u = x + phase;
      on_line = u - kDashPeriod * hm_floorf(u / kDashPeriod) < kDashOn;
    }
    col[j] = (in_x && on_line) ? c_line : ((in_x && row.surface) ? c_road : c_bg);
    if (++c == W) {
      c = 0;
      ++r;
      row = row_of(r, ch_h, scaling, ye, p.lanes_count);
    }
  }

  // layers 4-5: the survivors in painter's order
  for (int k = 0; k < n; ++k) {
    const float cx = s_cx[k], cy = s_cy[k], ch = s_ch[k], sh = s_sh[k];
    const uint32_t vc = s_col[k];
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
      const float dx = px[j] - cx, dy = py[j] - cy;
      const bool covered = hm_absf(dx * ch + dy * sh) <= kHalfLength &&
                           hm_absf(dy * ch - dx * sh) <= kHalfWidth;
      col[j] = covered ? vc : col[j];
    }
  }

  const size_t frame_bytes = (size_t)HW * (size_t)C;
  uint8_t* const fbase = p.a.frames + (size_t)frame * frame_bytes;
  uint8_t* const dst = fbase + (size_t)pix * (size_t)C;
  const int npix = HW - pix < kGroup ? HW - pix : kGroup;
  if (npix == kGroup && ((uintptr_t)fbase & 15u) == 0) {  // pix * C is a multiple of 16
    uint4* const d4 = reinterpret_cast<uint4*>(dst);
    if (luma) {
      uint32_t w[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        w[q] = col[4 * q] | (col[4 * q + 1] << 8) | (col[4 * q + 2] << 16) | (col[4 * q + 3] << 24);
      d4[0] = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      uint32_t w[12];
#pragma unroll
      for (int q = 0; q < 4; ++q) {  // four pixels -> three words
        const uint32_t a = col[4 * q], b = col[4 * q + 1], cc = col[4 * q + 2], d = col[4 * q + 3];
        w[3 * q] = a | (b << 24);
        w[3 * q + 1] = (b >> 8) | (cc << 16);
        w[3 * q + 2] = (cc >> 16) | (d << 8);
      }
      d4[0] = make_uint4(w[0], w[1], w[2], w[3]);
      d4[1] = make_uint4(w[4], w[5], w[6], w[7]);
      d4[2] = make_uint4(w[8], w[9], w[10], w[11]);
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < kGroup; ++j) {
    if (j < npix) {
      if (luma) {
        dst[j] = (uint8_t)col[j];
      } else {
        dst[3 * j] = (uint8_t)col[j];
        dst[3 * j + 1] = (uint8_t)(col[j] >> 8);
        dst[3 * j + 2] = (uint8_t)(col[j] >> 16);
      }
    }
  }
}

extern "C" int hwy_launch_render(const RenderParams* p, hipStream_t s) {
  const int bands = (p->a.width * p->a.height + kBlockPixels - 1) / kBlockPixels;
  hipLaunchKernelGGL(hwy_render_kernel, dim3((unsigned)p->a.n, (unsigned)bands), dim3(kThreads), 0,
                     s, *p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
