// The radar readout of every kept detection, on the device: how far away is the vessel in this box, and what do the radar
// points on it say.  The points of an image are projected through the camera matrix of its view record into continuous
// pixel coordinates of the ORIGINAL frame -- where the rows of FrameResult live too, so there is no window here -- and every
// box gets the number of points inside it, the nearest of them and their lower median by depth.  The reference has no code
// for this, as it has none for the radar map; the rule is this project's definition, stated on the host by data.box_radar,
// which these kernels equal bit for bit.
//
// Per point (x, y, z, f0..f3) of image b, in float32 with one rounding per operation (contraction off; radarpoint.h):
//   hu = ((P00 x + P01 y) + P02 z) + P03, hv and hw from rows 1 and 2; kept when hw >= min_depth and all three are finite
//   u = hu / hw, v = hv / hw; in view when 0 <= u < float(iw) and 0 <= v < float(ih)
// Per box (t, l, b, rt) = the first four numbers of its row:
//   shrink == 1: y0 = t, y1 = b, x0 = l, x1 = rt, the row's own numbers
//   otherwise    cy = (t + b) 0.5, cx = (l + rt) 0.5, hy = ((b - t) 0.5) shrink, hx = ((rt - l) 0.5) shrink,
//                y0 = cy - hy, y1 = cy + hy, x0 = cx - hx, x1 = cx + hx
//   inside when x0 <= u < x1 and y0 <= v < y1 (a NaN edge contains nothing)
// The candidates of a box are ordered by key = bits(hw) << 32 | index (rm_key): hw is positive and finite, so its bits order
// as an unsigned integer, and the index breaks ties.  count = their number; readout[0] = (hw, f0..f3) of the smallest key,
// readout[1] = the same of the key of rank (count - 1) / 2; feature BITS are copied; all ten numbers +0.0 without a candidate.
// Launches (grid y = image, the record loaded wave-uniformly):
//   project  one thread per point: (u, v, hw) into three planes of the workspace, hw = +0.0 for a point that is not kept, not
//            in view or past the image's count.  Every slot of the workspace is written, so no call sees an earlier one
//   select   one workgroup of 256 per (row, image).  Rows from kept[b] on write zeros and leave.  A first sweep over the
//            image's points gives the count and the minimum key (wave shuffles, then LDS across the four waves).  From three
//            candidates on the median is an MSB-first radix select on the 64-bit key, eight bits per pass: a 256-bin LDS
//            histogram of the candidates that still match the prefix (integer LDS atomics), a scan by wave 0 that picks
//            the bin of the wanted rank, narrowing of prefix and rank.  A bin of ONE candidate ends the passes: a last sweep
//            names the only key under the prefix.  Every pass re-reads the planes (12 bytes a point: they stay in L2);
//            there is no list of candidates anywhere, so no capacity at which the answer could change.  The winners'
//            features are gathered from `points` by index at the end.
// Integer atomics only (the one global atomic is the OR into *flag), counts and exact selections: the same bytes on every run.
#include "radarpoint.h"
#include "wgscan.h"

#pragma clang fp contract(off)

extern "C" {
/* include/vrnet_hip.h: the per-image view record of the radar map (80 bytes); ih, iw, count and P are read here. */
typedef struct vrnet_radar_view {
  int ih, iw;
  int nw, nh, dx, dy;
  int flip, count;
  float P[12];
} vrnet_radar_view;
}
static_assert(sizeof(vrnet_radar_view) == 80 && alignof(vrnet_radar_view) == 4, "vrnet_radar_view layout");

namespace {

constexpr int BR_ROW_FLOATS = 7;     // top, left, bottom, right, obj, class_conf, class
constexpr int BR_OUT_FLOATS = 10;    // (hw, f0..f3) of the nearest, then of the median

struct BoxRadarArgs {
  const float* points;               // (B, max_points, 7)
  const vrnet_radar_view* views;     // (B)
  const float* rows;                 // (B, cap, 7)
  const int* kept;                   // (B)
  int B, max_points, cap;
  float min_depth, shrink;
  float *u, *v, *hw;                 // the workspace: three planes (B, max_points)
  int* counts;                       // (B, cap)
  unsigned* readout;                 // (B, cap, 2, 5), written as bits
  int* flag;                         // or null
};

__global__ __launch_bounds__(256) void box_radar_project_kernel(const BoxRadarArgs p) {
  const int b = blockIdx.y;
  const vrnet_radar_view g = p.views[b];
  const bool bad = g.ih <= 0 || g.iw <= 0;
  const int count = vr_clampi(g.count, 0, p.max_points);
  if (blockIdx.x == 0 && threadIdx.x == 0 && p.flag) {
    const int bits = (bad ? VR_FLAG_GEOMETRY : 0) | (count != g.count ? VR_FLAG_POINT_COUNT : 0);
    if (bits) atomicOr(p.flag, bits);
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.max_points) return;
  const long at = (long)b * p.max_points + i;
  float u = 0.f, v = 0.f, hw = 0.f;
  if (!bad && i < count) {
    float pu, pv, ph;
    if (rm_project_uv(g.P, p.points + at * RM_POINT_FLOATS, p.min_depth, pu, pv, ph) &&      // radarpoint.h
        pu >= 0.f && pu < (float)g.iw && pv >= 0.f && pv < (float)g.ih) {
      u = pu;  v = pv;  hw = ph;
    }
  }
  p.u[at] = u;
  p.v[at] = v;
  p.hw[at] = hw;
}

// the candidates of this box among the image's n projected points whose key equals `prefix` on the bits of `mask`: their
// number and their smallest key, the same in every thread.  red_n / red_k: four slots each; ends behind a barrier
__device__ __forceinline__ void br_sweep(const float* pu, const float* pv, const float* ph, int n, float x0, float x1, float y0,
                                         float y1, unsigned long long mask, unsigned long long prefix, int* red_n,
                                         unsigned long long* red_k, int& count, unsigned long long& best) {
  int c = 0;
  unsigned long long k = RM_EMPTY;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float h = ph[i];
    const unsigned long long key = rm_key(h, i);
    if (!(h > 0.f) || (key & mask) != prefix) continue;
    const float u = pu[i], v = pv[i];
    if (x0 <= u && u < x1 && y0 <= v && v < y1) {
      ++c;
      k = key < k ? key : k;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = vr_shfl_xor64(k, o);
    k = t < k ? t : k;
  }
  __syncthreads();                     // the slots may still be read from the sweep before
  if ((threadIdx.x & 63) == 0) red_k[threadIdx.x >> 6] = k;
  count = vr_block_sum(c, red_n);      // its barrier stands behind the keys too
  best = red_k[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) best = red_k[w] < best ? red_k[w] : best;
}

__global__ __launch_bounds__(256) void box_radar_select_kernel(const BoxRadarArgs p) {
  __shared__ unsigned hist[256];
  __shared__ int red_n[4];
  __shared__ unsigned long long red_k[4];
  __shared__ int pick[3];              // the bin of the wanted rank, the candidates in front of it, its own count
  const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const vrnet_radar_view g = p.views[b];
  const int raw_kept = p.kept[b];
  const int kept = vr_clampi(raw_kept, 0, p.cap);
  if (r == 0 && tid == 0 && p.flag && kept != raw_kept) atomicOr(p.flag, VR_FLAG_BOX_COUNT);
  const long row = (long)b * p.cap + r;
  const int n = (g.ih <= 0 || g.iw <= 0) ? 0 : vr_clampi(g.count, 0, p.max_points);
  int count = 0;
  unsigned long long nearest = RM_EMPTY, median = RM_EMPTY;
  if (r < kept && n > 0) {             // wave-uniform, and so is every branch below: count and pick come from LDS
    const float* q = p.rows + row * BR_ROW_FLOATS;
    const float t = q[0], l = q[1], bo = q[2], rt = q[3];
    float y0 = t, y1 = bo, x0 = l, x1 = rt;
    if (p.shrink != 1.f) {
      const float cy = (t + bo) * 0.5f, cx = (l + rt) * 0.5f;
      const float hy = ((bo - t) * 0.5f) * p.shrink, hx = ((rt - l) * 0.5f) * p.shrink;
      y0 = cy - hy;  y1 = cy + hy;  x0 = cx - hx;  x1 = cx + hx;
    }
    const long base = (long)b * p.max_points;
    const float *pu = p.u + base, *pv = p.v + base, *ph = p.hw + base;
    br_sweep(pu, pv, ph, n, x0, x1, y0, y1, 0ULL, 0ULL, red_n, red_k, count, nearest);
    median = nearest;                  // rank (count - 1) / 2 is 0 up to two candidates
    if (count >= 3) {
      int rank = (count - 1) >> 1, left = count;
      unsigned long long mask = 0ULL, prefix = 0ULL;
      for (int shift = 56; shift >= 0 && left > 1; shift -= 8) {
        hist[tid] = 0u;
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
          const float h = ph[i];
          const unsigned long long key = rm_key(h, i);
          if (!(h > 0.f) || (key & mask) != prefix) continue;
          const float u = pu[i], v = pv[i];
          if (x0 <= u && u < x1 && y0 <= v && v < y1) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {                // four bins a lane, an inclusive scan over the lanes, one lane holds the rank
          unsigned h4[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) h4[j] = hist[4 * tid + j];
          const unsigned own = (h4[0] + h4[1]) + (h4[2] + h4[3]);
          const unsigned incl = vr_wave_scan_incl(own);
          unsigned before = incl - own, sel = h4[0];
          if ((unsigned)rank >= before && (unsigned)rank < incl) {
            int j = 0;
#pragma unroll
            for (int s = 1; s < 4; ++s)
              if (j == s - 1 && (unsigned)rank >= before + sel) {
                before += sel;
                sel = h4[s];
                j = s;
              }
            pick[0] = 4 * tid + j;
            pick[1] = (int)before;
            pick[2] = (int)sel;
          }
        }
        __syncthreads();               // the next pass writes hist and pick behind two more barriers
        prefix |= (unsigned long long)(unsigned)pick[0] << shift;
        mask |= 0xFFULL << shift;
        rank -= pick[1];
        left = pick[2];
      }
      if (mask == ~0ULL) {
        median = prefix;               // all 64 bits chosen
      } else {                         // one candidate is left under the prefix: name it
        int one;
        br_sweep(pu, pv, ph, n, x0, x1, y0, y1, mask, prefix, red_n, red_k, one, median);
      }
    }
  }
  if (tid == 0) p.counts[row] = count;
  if (tid < BR_OUT_FLOATS) {
    const unsigned long long key = tid < 5 ? nearest : median;
    const int c = tid < 5 ? tid : tid - 5;
    unsigned bits = 0u;
    if (count > 0 && key != RM_EMPTY) {
      const unsigned idx = (unsigned)key < (unsigned)p.max_points ? (unsigned)key : 0u;     // a key's index is below n
      bits = c == 0 ? (unsigned)(key >> 32)
                    : reinterpret_cast<const unsigned*>(p.points)[((long)b * p.max_points + idx) * RM_POINT_FLOATS + 2 + c];
    }
    p.readout[row * BR_OUT_FLOATS + tid] = bits;
  }
}

long box_radar_bytes(int B, int max_points) { return vr_align256((long)B * max_points * 12); }

}  // namespace

extern "C" long vrnet_box_radar_workspace(int B, int max_points) {
  if (B <= 0 || B >= 65536 || max_points <= 0 || max_points > (1 << 24)) return -1;
  return box_radar_bytes(B, max_points);
}

extern "C" int vrnet_box_radar_f32(const float* points, int max_points, const vrnet_radar_view* views, int B, const float* rows,
                                   const int* kept, int cap, float min_depth, float shrink, int* counts_out, float* readout_out,
                                   int* flag, void* workspace, long workspace_bytes, void* stream) {
  const char* who = "box_radar";
  VR_CHECK_ARG(points && views && rows && kept && counts_out && readout_out,
               "%s: points, views, rows, kept, counts_out and readout_out are required", who);
  VR_CHECK_ARG(B > 0 && B < 65536 && max_points > 0 && max_points <= (1 << 24) && cap > 0 && cap <= (1 << 20),
               "%s: bad shape (B %d, max_points %d, cap %d)", who, B, max_points, cap);
  VR_CHECK_ARG(min_depth > 0.f && min_depth < INFINITY, "%s: min_depth must be positive and finite, got %g", who,
               (double)min_depth);
  VR_CHECK_ARG(shrink > 0.f && shrink <= 1.f, "%s: shrink must lie in (0, 1], got %g", who, (double)shrink);
  VR_CHECK_ARG((reinterpret_cast<uintptr_t>(views) & 7) == 0, "%s: the view table must be 8-byte aligned", who);
  const long need = box_radar_bytes(B, max_points);
  if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7)) {
    vr_set_error("%s: workspace %ld < %ld bytes, or not 8-byte aligned", who, workspace ? workspace_bytes : 0L, need);
    return VR_ERR_WORKSPACE;
  }
  BoxRadarArgs p{};
  p.points = points; p.views = views; p.rows = rows; p.kept = kept;
  p.B = B; p.max_points = max_points; p.cap = cap;
  p.min_depth = min_depth; p.shrink = shrink;
  p.u = static_cast<float*>(workspace);
  p.v = p.u + (long)B * max_points;
  p.hw = p.v + (long)B * max_points;
  p.counts = counts_out;
  p.readout = reinterpret_cast<unsigned*>(readout_out);
  p.flag = flag;
  hipStream_t st = vr_stream(stream);
  hipLaunchKernelGGL(box_radar_project_kernel, dim3((unsigned)vr_cdiv(max_points, 256), B), dim3(256), 0, st, p);
  hipLaunchKernelGGL(box_radar_select_kernel, dim3((unsigned)cap, B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK(who);
  return VR_OK;
}
