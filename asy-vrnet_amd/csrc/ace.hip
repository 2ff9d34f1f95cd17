// Fast Automatic Colour Equalisation (ACE) of raw frames on the device: the de-rain enhancement of the reference's
// image_augmentation_test/sharpen.py restated; the host statement is render.ace_host, and the kernels equal it byte for byte.
//
// THE RULE, for one (ih, iw, 3) uint8 image, each channel on its own; every float64 operation is rounded on its own, in the
// order written (nothing is contracted, divisions are IEEE).  Parameters ratio, radius, s, bins; m: the (2 radius + 1)^2 tap
// weights, computed on the host (render.ace_weights: 1 / sqrt(dy^2 + dx^2), centre 0, normalised) and passed as data.
//   I_0      = double(byte) / 255.0
//   ice(P)   : res = 0.0; for dy = -radius .. radius and, inside it, dx = -radius .. radius, without the centre:
//              res += m[dy, dx] * clip((P(y, x) - P(cy, cx)) * ratio, -1, 1), cy = clamp(y + dy, 0, h - 1), cx likewise
//   resize(S, h, w), cv2's default INTER_LINEAR on float64: a source of exactly (2 h, 2 w) takes OpenCV's exact-halving
//              switch to the area path, (((S00 + S01) + S10) + S11) * 0.25 over each 2 x 2 block.  Otherwise per axis, for
//              destination index d, source length n, destination length k: scale = double(n) / double(k);
//              f = float((d + 0.5) * scale - 0.5); s0 = floor(f); f -= s0 (float); s0 < 0: s0 = 0, f = 0; s0 >= n - 1:
//              s0 = n - 1, f = 0; s1 = min(s0 + 1, n - 1); a0 = double(1.f - f), a1 = double(f).  Columns first:
//              H(y, x) = S(y, x0) * a0 + S(y, x1) * a1; then rows: out = H(y0, x) * b0 + H(y1, x) * b1
//   pyramid  : I_{L+1} = resize(I_L, (h_L + 1) / 2, (w_L + 1) / 2) while min(h_L, w_L) > 2; at the first level with
//              min <= 2 (the bottom) R = 0.5 everywhere; above it
//              R_L = (resize(R_{L+1}, h_L, w_L) + ice(I_L)) - ice(resize(I_{L+1}, h_L, w_L)).  The constant bottom goes
//              through the resize formula like any plane
//   stretch  : first, last = min, max of R_0 (equal: widened by 0.5 each way); step = (last - first) / bins;
//              edge(i) = i * step + first, edge(bins) = last; the bin of v: idx = int(((v - first) / (last - first)) * bins),
//              idx == bins: idx -= 1; v < edge(idx): idx -= 1; v >= edge(idx + 1) and idx != bins - 1: idx += 1 (numpy's
//              uniform-bin rule); d(i) = double(cumulative count) / double(ih iw); lmin = the first i with d(i) >= s;
//              lmax = the last i with d(i) <= 1.0 - s, or -1; out = clip((R_0 - edge(lmin)) / (edge(lmax) - edge(lmin)), 0, 1);
//              byte = clip(rint(out * 255.0), 0, 255), half to even
// DEGENERATE: min(ih, iw) <= 2, or lmax <= lmin in any channel.  All three channels of such an image come back unchanged and
// VR_FLAG_ACE is set.  A geometry record with ih, iw <= 0 or above the slot sets VR_FLAG_GEOMETRY and gives a zero image.
// Outside an image's corner of its slot out is 0.
//
// THE LAUNCHES (one body each for fixed-size batches and geometry tables), 2 N + 4 for a slot whose pyramid has N levels above
// its bottom (N = 10 at 1080 x 1920: 24).  The grids follow (B, ihm, iwm) alone; every image derives its level sizes from its
// own record, and workgroups beyond an image's level, or at and below its bottom, leave at once.
//   ace_init         per image: the record (size, bottom level), the histograms zeroed, the minimum / maximum keys reset
//   ace_down  x N    I_{L+1} from I_L (level 0 from the bytes)
//   ace_level x N    from the deepest level up.  Per 32 x 32 tile and channel: the tile of I_L and the tile of
//                    resize(I_{L+1}) in LDS, each with a halo of radius whose coordinates are clamped to the level's extent
//                    BEFORE they are evaluated -- so the second tile holds the up-resized plane's own edge pixels --, both
//                    tap sums from LDS (four outputs per thread, rows of one column: independent chains that share their
//                    LDS reads), the tap weights through the scalar cache, resize(R_{L+1}) at the pixel, R_L stored.  One
//                    instance per radius 1 .. 8.  No full-size plane of either up-resized operand exists.  Level 0 also folds the
//                    minimum and maximum of R_0 into two order-preserving 64-bit integer keys per channel (integer atomics)
//   ace_hist         the bins of R_0 by the rule above: LDS integer atomics, then one global integer atomic per non-empty bin
//   ace_scan         per image: the cumulative counts, lmin, lmax and the two edges of each channel, the degenerate decision,
//                    the flag
//   ace_store        the whole slot: the stretch and the byte store, the unchanged degenerate images, the zeros outside
// Integer atomics only: the same bytes on every run.  Every call initialises what it accumulates into.  No allocation, no
// memset node, no host synchronisation.
//
// WORKSPACE (vrnet_ace_workspace_bytes): per image a record, six keys, six doubles (edge(lmin) and the edge difference per
// channel) and 3 x 4096 histogram bins; then R_0 and, for every deeper level of the SLOT's pyramid, I_L and R_L, each
// (B, 3, hm_L, wm_L) float64 with hm_{L+1} = (hm_L + 1) / 2: about 5 / 3 planes of 3 B ihm iwm doubles.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int ACE_MAXR = 8, ACE_MAXBINS = 4096, ACE_MAXLEVELS = 20;
constexpr int ACE_T = 32;                                     // the level kernel's tile, ACE_T x ACE_T
constexpr int ACE_HW = 256, ACE_HH = 64;                      // the histogram's block of R_0
constexpr int ACE_BAD = 1, ACE_DEGENERATE = 2;                // bits of AceRec::state

struct AceRec {                     // the integer record of one image
  int state, ih, iw, nl;            // nl: the index of the bottom level (0: the image itself is the bottom)
};

struct AceLevel {                   // one level of the slot's pyramid
  double* I;                        // (B, 3, hm, wm); NULL at level 0, whose plane is the bytes
  double* R;                        // (B, 3, hm, wm)
  int hm, wm;
};

struct AceArgs {
  const unsigned char* frames;      // (B, ihm, iwm, 3)
  const vrnet_frame_geom* geom;     // (B) or NULL
  unsigned char* out;               // (B, ihm, iwm, 3)
  int* flag;
  AceRec* rec;                      // (B)
  unsigned long long* keys;         // (B, 3, 2): the minimum and the maximum of R_0 as ordered keys
  double* recd;                     // (B, 8): edge(lmin) of the channels, then edge(lmax) - edge(lmin)
  int* hist;                        // (B, 3, ACE_MAXBINS)
  double ratio, s;
  int ihm, iwm, bins;
};

struct AceTap {
  int s0, s1;
  double a0, a1;
};

// the two taps of destination index d on an axis of source length n and destination length k
__device__ __forceinline__ AceTap ace_tap(int d, int n, int k) {
  const double scale = (double)n / (double)k;
  const double pos = ((double)d + 0.5) * scale;
  float f = (float)(pos - 0.5);
  const float fl = floorf(f);
  int s0 = (int)fl;
  f -= fl;
  if (s0 < 0) {
    s0 = 0;
    f = 0.f;
  }
  if (s0 >= n - 1) {
    s0 = n - 1;
    f = 0.f;
  }
  AceTap t;
  t.s0 = s0;
  t.s1 = min(s0 + 1, n - 1);
  t.a0 = (double)(1.f - f);
  t.a1 = (double)f;
  return t;
}

__device__ __forceinline__ void ace_level_size(const AceRec& rec, int L, int& h, int& w) {
  h = rec.ih;
  w = rec.iw;
  for (int i = 0; i < L; ++i) {
    h = (h + 1) >> 1;
    w = (w + 1) >> 1;
  }
}

// doubles <-> unsigned keys of the same order
__device__ __forceinline__ unsigned long long ace_key(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v + 0.0);      // -0.0 -> +0.0
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ace_unkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// clip(d, -1, 1) of a finite d
__device__ __forceinline__ double ace_clip1(double d) { return __builtin_fmin(__builtin_fmax(d, -1.0), 1.0); }

__global__ __launch_bounds__(256) void ace_init_kernel(const AceArgs p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < 3 * ACE_MAXBINS; i += 256) p.hist[(long)b * 3 * ACE_MAXBINS + i] = 0;
  if (tid < 3) {
    p.keys[(b * 3 + tid) * 2] = ~0ull;
    p.keys[(b * 3 + tid) * 2 + 1] = 0ull;
  }
  if (tid < 8) p.recd[b * 8 + tid] = 0.0;
  if (tid == 0) {
    int ih, iw;
    bool bad;
    vr_image_size(p.geom, b, p.ihm, p.iwm, p.ihm, p.iwm, ih, iw, bad);
    int state = 0, nl = 0;
    if (bad) {
      state = ACE_BAD;
      ih = iw = 0;
    } else {
      for (int h = ih, w = iw; min(h, w) > 2; h = (h + 1) >> 1, w = (w + 1) >> 1) ++nl;
      if (nl == 0) state = ACE_DEGENERATE;
    }
    p.rec[b] = AceRec{state, ih, iw, nl};
  }
}

// I_{L+1} (dst) from I_L (src; the bytes at L = 0): 32 x 8 outputs per workgroup, the channel folded into blockIdx.x
__global__ __launch_bounds__(256) void ace_down_kernel(const AceArgs p, const AceLevel src, const AceLevel dst, int L) {
  const int b = blockIdx.z;
  const AceRec rec = p.rec[b];
  if (rec.state || L + 1 > rec.nl) return;                                       // workgroup-uniform
  const int tiles = (dst.wm + 31) / 32, c = blockIdx.x / tiles;
  const int x = (blockIdx.x - c * tiles) * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
  int h, w;
  ace_level_size(rec, L, h, w);
  const int h1 = (h + 1) >> 1, w1 = (w + 1) >> 1;
  if (x >= w1 || y >= h1) return;
  const unsigned char* bytes = p.frames + 3L * b * p.ihm * p.iwm + c;
  const double* plane = src.I ? src.I + ((long)b * 3 + c) * src.hm * src.wm : nullptr;
  auto S = [&](int yy, int xx) -> double {
    return plane ? plane[(long)yy * src.wm + xx] : (double)bytes[3L * ((long)yy * p.iwm + xx)] / 255.0;
  };
  double v;
  if (!(h & 1) && !(w & 1)) {
    const double s00 = S(2 * y, 2 * x), s01 = S(2 * y, 2 * x + 1), s10 = S(2 * y + 1, 2 * x), s11 = S(2 * y + 1, 2 * x + 1);
    v = (((s00 + s01) + s10) + s11) * 0.25;
  } else {
    const AceTap tx = ace_tap(x, w, w1), ty = ace_tap(y, h, h1);
    const double h0 = S(ty.s0, tx.s0) * tx.a0 + S(ty.s0, tx.s1) * tx.a1;
    const double h1v = S(ty.s1, tx.s0) * tx.a0 + S(ty.s1, tx.s1) * tx.a1;
    v = h0 * ty.a0 + h1v * ty.a1;
  }
  dst.I[(((long)b * 3 + c) * dst.hm + y) * dst.wm + x] = v;
}

// R_L of one tile and channel: thread (cx, rg) owns the outputs (y0 + 4 rg + k, x0 + cx), k = 0 .. 3, four rows of one column.
// It walks the source rows s = -r .. 3 + r of that column once: the value at (s, dx) is the tap (dy = s - k, dx) of output k,
// so each LDS read serves up to four outputs, and every output still meets its taps in the order of the rule (dy, then dx).
// The radius is a template argument: the row segment of 2 R + 1 taps sits in registers, the dx loop is unrolled, and the
// weights -- a wave-uniform row of the table per (s, k) -- come through scalar loads, not through LDS.
template <int RADIUS>
__global__ __launch_bounds__(256) void ace_level_kernel(const AceArgs p, const AceLevel cur, const AceLevel nxt, int L,
                                                        const double* __restrict__ wts) {
  constexpr int r = RADIUS, sw = ACE_T + 2 * r, nw = 2 * r + 1;
  __shared__ double s_a[sw * sw];                   // I_L with its halo
  __shared__ double s_b[sw * sw];                   // resize(I_{L+1}) with its halo
  __shared__ double s_lut[256];                     // level 0: double(byte) / 255.0, the division once per byte value
  __shared__ double s_xa0[sw], s_xa1[sw], s_ya0[sw], s_ya1[sw];
  __shared__ int s_x0[sw], s_x1[sw], s_y0[sw], s_y1[sw], s_cx[sw], s_cy[sw];
  __shared__ unsigned long long s_lo[4], s_hi[4];
  const int b = blockIdx.z, tid = threadIdx.x;
  const AceRec rec = p.rec[b];
  if (rec.state || L >= rec.nl) return;                                          // workgroup-uniform
  const int tiles = (cur.wm + ACE_T - 1) / ACE_T, c = blockIdx.x / tiles;
  const int x0 = (blockIdx.x - c * tiles) * ACE_T, y0 = blockIdx.y * ACE_T;
  int h, w;
  ace_level_size(rec, L, h, w);
  if (x0 >= w || y0 >= h) return;                                                // workgroup-uniform
  const int h1 = (h + 1) >> 1, w1 = (w + 1) >> 1;
  // the halo's coordinates, clamped to the level, and their taps into level L + 1
  if (tid < sw) {
    const int gx = vr_clampi(x0 - r + tid, 0, w - 1);
    const AceTap t = ace_tap(gx, w1, w);
    s_cx[tid] = gx;
    s_x0[tid] = t.s0;
    s_x1[tid] = t.s1;
    s_xa0[tid] = t.a0;
    s_xa1[tid] = t.a1;
  } else if (tid >= 64 && tid < 64 + sw) {
    const int e = tid - 64, gy = vr_clampi(y0 - r + e, 0, h - 1);
    const AceTap t = ace_tap(gy, h1, h);
    s_cy[e] = gy;
    s_y0[e] = t.s0;
    s_y1[e] = t.s1;
    s_ya0[e] = t.a0;
    s_ya1[e] = t.a1;
  }
  s_lut[tid] = (double)tid / 255.0;
  __syncthreads();
  const unsigned char* bytes = p.frames + 3L * b * p.ihm * p.iwm + c;
  const double* planeI = cur.I ? cur.I + ((long)b * 3 + c) * cur.hm * cur.wm : nullptr;
  const double* nextI = nxt.I + ((long)b * 3 + c) * nxt.hm * nxt.wm;
  for (int i = tid; i < sw * sw; i += 256) {
    const int ly = i / sw, lx = i - ly * sw;
    const int gy = s_cy[ly], gx = s_cx[lx];
    s_a[i] = planeI ? planeI[(long)gy * cur.wm + gx] : s_lut[bytes[3L * ((long)gy * p.iwm + gx)]];
    const double* row0 = nextI + (long)s_y0[ly] * nxt.wm;
    const double* row1 = nextI + (long)s_y1[ly] * nxt.wm;
    const double a0 = s_xa0[lx], a1 = s_xa1[lx];
    const double u0 = row0[s_x0[lx]] * a0 + row0[s_x1[lx]] * a1;
    const double u1 = row1[s_x0[lx]] * a0 + row1[s_x1[lx]] * a1;
    s_b[i] = u0 * s_ya0[ly] + u1 * s_ya1[ly];
  }
  __syncthreads();
  const int cx = tid & 31, rg = tid >> 5;
  double pa[4], pb[4], ra[4], rb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int at = (4 * rg + k + r) * sw + cx + r;
    pa[k] = s_a[at];
    pb[k] = s_b[at];
    ra[k] = 0.0;
    rb[k] = 0.0;
  }
  const double ratio = p.ratio;
#pragma unroll 1
  for (int s = -r; s <= 3 + r; ++s) {               // tile row 4 rg + s + r lies in 0 .. 31 + 2 r, columns cx .. cx + 2 r
    const int row = (4 * rg + s + r) * sw + cx;
    double qa[nw], qb[nw];
#pragma unroll
    for (int j = 0; j < nw; ++j) {
      qa[j] = s_a[row + j];
      qb[j] = s_b[row + j];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int dy = s - k;                         // wave-uniform, like everything these branches read
      if (dy < -r || dy > r) continue;
      const double* wrow = wts + (dy + r) * nw;
#pragma unroll
      for (int j = 0; j < nw; ++j) {
        if (j == r && dy == 0) continue;            // the centre
        const double m = wrow[j];
        const double da = ace_clip1((pa[k] - qa[j]) * ratio), db = ace_clip1((pb[k] - qb[j]) * ratio);
        const double ta = m * da, tb = m * db;
        ra[k] += ta;
        rb[k] += tb;
      }
    }
  }
  // resize(R_{L+1}) at the pixel; the bottom level is the constant 0.5, which goes through the same formula
  const bool bottom = L + 1 == rec.nl;
  const double* nextR = nxt.R + ((long)b * 3 + c) * nxt.hm * nxt.wm;
  double* outR = cur.R + ((long)b * 3 + c) * cur.hm * cur.wm;
  const int x = x0 + cx;
  unsigned long long lo = ~0ull, hi = 0ull;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = 4 * rg + k, y = y0 + ly;
    if (y < h && x < w) {
      const int ex = cx + r, ey = ly + r;           // the pixel's own entries of the tap tables
      double v00 = 0.5, v01 = 0.5, v10 = 0.5, v11 = 0.5;
      if (!bottom) {
        const double* row0 = nextR + (long)s_y0[ey] * nxt.wm;
        const double* row1 = nextR + (long)s_y1[ey] * nxt.wm;
        v00 = row0[s_x0[ex]];
        v01 = row0[s_x1[ex]];
        v10 = row1[s_x0[ex]];
        v11 = row1[s_x1[ex]];
      }
      const double u0 = v00 * s_xa0[ex] + v01 * s_xa1[ex];
      const double u1 = v10 * s_xa0[ex] + v11 * s_xa1[ex];
      const double up = u0 * s_ya0[ey] + u1 * s_ya1[ey];
      const double R = (up + ra[k]) - rb[k];
      outR[(long)y * cur.wm + x] = R;
      const unsigned long long key = ace_key(R);
      lo = key < lo ? key : lo;
      hi = key > hi ? key : hi;
    }
  }
  if (L == 0) {                                     // launch-uniform: every thread of the workgroup is still here
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long ol = __shfl_xor(lo, o, 64), oh = __shfl_xor(hi, o, 64);
      lo = ol < lo ? ol : lo;
      hi = oh > hi ? oh : hi;
    }
    if ((tid & 63) == 0) {
      s_lo[tid >> 6] = lo;
      s_hi[tid >> 6] = hi;
    }
    __syncthreads();
    if (tid == 0) {
      for (int i = 1; i < 4; ++i) {
        lo = s_lo[i] < lo ? s_lo[i] : lo;
        hi = s_hi[i] > hi ? s_hi[i] : hi;
      }
      atomicMin(&p.keys[(b * 3 + c) * 2], lo);
      atomicMax(&p.keys[(b * 3 + c) * 2 + 1], hi);
    }
  }
}

// first, last and step of a channel's histogram from its keys
__device__ __forceinline__ void ace_range(const AceArgs& p, int b, int c, double& first, double& last, double& step) {
  first = ace_unkey(p.keys[(b * 3 + c) * 2]);
  last = ace_unkey(p.keys[(b * 3 + c) * 2 + 1]);
  if (first == last) {
    first = first - 0.5;
    last = last + 0.5;
  }
  step = (last - first) / (double)p.bins;
}

__global__ __launch_bounds__(256) void ace_hist_kernel(const AceArgs p, const AceLevel lv) {
  __shared__ int s_hist[ACE_MAXBINS];
  const int b = blockIdx.z, tid = threadIdx.x;
  const AceRec rec = p.rec[b];
  if (rec.state) return;                                                         // workgroup-uniform
  const int tiles = (p.iwm + ACE_HW - 1) / ACE_HW, c = blockIdx.x / tiles;
  const int x = (blockIdx.x - c * tiles) * ACE_HW + tid, y0 = blockIdx.y * ACE_HH;
  if ((blockIdx.x - c * tiles) * ACE_HW >= rec.iw || y0 >= rec.ih) return;       // workgroup-uniform
  const int bins = p.bins;
  for (int i = tid; i < bins; i += 256) s_hist[i] = 0;
  __syncthreads();
  double first, last, step;
  ace_range(p, b, c, first, last, step);
  const double range = last - first, nb = (double)bins;
  if (x < rec.iw) {
    const double* R = lv.R + ((long)b * 3 + c) * lv.hm * lv.wm;
    const int y1 = min(y0 + ACE_HH, rec.ih);
    for (int y = y0; y < y1; ++y) {
      const double v = R[(long)y * lv.wm + x];
      const double q = (v - first) / range;
      int idx = vr_clampi((int)(q * nb), 0, bins);
      if (idx == bins) --idx;
      const double e0 = (double)idx * step + first;
      if (v < e0) --idx;
      idx = max(idx, 0);
      const double e1 = idx + 1 == bins ? last : (double)(idx + 1) * step + first;
      if (v >= e1 && idx != bins - 1) ++idx;
      atomicAdd(&s_hist[idx], 1);
    }
  }
  __syncthreads();
  for (int i = tid; i < bins; i += 256) {
    const int n = s_hist[i];
    if (n) atomicAdd(&p.hist[((long)b * 3 + c) * ACE_MAXBINS + i], n);
  }
}

__global__ __launch_bounds__(256) void ace_scan_kernel(const AceArgs p) {
  __shared__ int s_part[256];
  __shared__ int s_lmin, s_lmax;
  const int b = blockIdx.x, tid = threadIdx.x;
  const AceRec rec = p.rec[b];
  if (rec.state) {                                                               // workgroup-uniform
    if (tid == 0 && p.flag) atomicOr(p.flag, (rec.state & ACE_BAD) ? VR_FLAG_GEOMETRY : VR_FLAG_ACE);
    return;
  }
  const int bins = p.bins, per = (bins + 255) / 256, i0 = tid * per, i1 = min(i0 + per, bins);
  const double n = (double)((long)rec.ih * rec.iw), top = 1.0 - p.s;
  bool degenerate = false;                                                       // read by thread 0 alone
  for (int c = 0; c < 3; ++c) {
    const int* hist = p.hist + ((long)b * 3 + c) * ACE_MAXBINS;
    int sum = 0;
    for (int i = i0; i < i1; ++i) sum += hist[i];
    s_part[tid] = sum;
    if (tid == 0) {
      s_lmin = bins;
      s_lmax = -1;
    }
    __syncthreads();
    long run = 0;
    for (int t = 0; t < tid; ++t) run += s_part[t];
    int lmin = bins, lmax = -1;
    for (int i = i0; i < i1; ++i) {
      run += hist[i];
      const double d = (double)run / n;
      if (d >= p.s && lmin == bins) lmin = i;
      if (d <= top) lmax = i;
    }
    if (lmin < bins) atomicMin(&s_lmin, lmin);
    if (lmax >= 0) atomicMax(&s_lmax, lmax);
    __syncthreads();
    if (tid == 0) {
      if (s_lmax <= s_lmin) {
        degenerate = true;
      } else {
        double first, last, step;
        ace_range(p, b, c, first, last, step);
        const double lo = (double)s_lmin * step + first, hi = (double)s_lmax * step + first;       // s_lmax <= bins - 1
        p.recd[b * 8 + c] = lo;
        p.recd[b * 8 + 3 + c] = hi - lo;
      }
    }
    __syncthreads();
  }
  if (tid == 0 && degenerate) {
    p.rec[b].state = ACE_DEGENERATE;
    if (p.flag) atomicOr(p.flag, VR_FLAG_ACE);
  }
}

// every pixel of the slot: 64 x 4 per workgroup
__global__ __launch_bounds__(256) void ace_store_kernel(const AceArgs p, const AceLevel lv) {
  const int b = blockIdx.z, x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= p.iwm || y >= p.ihm) return;
  const AceRec rec = p.rec[b];
  const long at = ((long)b * p.ihm + y) * p.iwm + x;
  unsigned int q[3] = {0u, 0u, 0u};
  if (y < rec.ih && x < rec.iw) {                                                // ih = iw = 0 for a bad record
    const unsigned char* px = p.frames + 3 * at;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      q[c] = px[c];
      if (rec.state == 0) {
        const double R = lv.R[(((long)b * 3 + c) * lv.hm + y) * lv.wm + x];
        double v = (R - p.recd[b * 8 + c]) / p.recd[b * 8 + 3 + c];
        v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
        double t = __builtin_rint(v * 255.0);
        t = t < 0.0 ? 0.0 : (t > 255.0 ? 255.0 : t);
        q[c] = (unsigned int)(int)t;
      }
    }
  }
  unsigned char* dst = p.out + 3 * at;
  dst[0] = (unsigned char)q[0];
  dst[1] = (unsigned char)q[1];
  dst[2] = (unsigned char)q[2];
}

struct AceLayout {
  long rec, keys, recd, hist, total;
  long I[ACE_MAXLEVELS], R[ACE_MAXLEVELS];
  int hm[ACE_MAXLEVELS], wm[ACE_MAXLEVELS];
  int nl;                           // the slot's bottom level
};
AceLayout ace_layout(int B, int ihm, int iwm) {
  AceLayout l;
  l.rec = 0;
  l.keys = vr_align256(l.rec + (long)sizeof(AceRec) * B);
  l.recd = vr_align256(l.keys + 48L * B);
  l.hist = vr_align256(l.recd + 64L * B);
  long at = vr_align256(l.hist + 12L * ACE_MAXBINS * B);
  l.nl = 0;
  l.hm[0] = ihm;
  l.wm[0] = iwm;
  while (l.hm[l.nl] > 2 && l.wm[l.nl] > 2) {
    l.hm[l.nl + 1] = (l.hm[l.nl] + 1) / 2;
    l.wm[l.nl + 1] = (l.wm[l.nl] + 1) / 2;
    ++l.nl;
  }
  for (int L = 0; L <= l.nl; ++L) {
    const long plane = vr_align256(24L * B * l.hm[L] * l.wm[L]);
    l.I[L] = -1;
    if (L > 0) {
      l.I[L] = at;
      at += plane;
    }
    l.R[L] = at;
    at += plane;
  }
  l.total = at;
  return l;
}
bool ace_shape_ok(int B, int ihm, int iwm) {
  return B > 0 && B < 65536 && ihm > 0 && iwm > 0 && ihm <= (1 << 17) && iwm <= (1 << 17) && (long)ihm * iwm <= (1L << 26) &&
         (long)B * ihm * iwm <= (1L << 31);
}

}  // namespace

extern "C" long vrnet_ace_workspace_bytes(int B, int ihm, int iwm) {
  if (!ace_shape_ok(B, ihm, iwm)) return -1;
  return ace_layout(B, ihm, iwm).total;
}

extern "C" int vrnet_ace_u8(const unsigned char* frames, const vrnet_frame_geom* geom, int B, int ihm, int iwm, int radius,
                            double ratio, double s, int bins, const double* weights, unsigned char* out, int* flag, void* workspace,
                            long workspace_bytes, void* stream) {
  VR_CHECK_ARG(frames && out && workspace && weights && frames != out,
               "ace: frames, out (a different buffer), the weights and the workspace are required");
  VR_CHECK_ARG(ace_shape_ok(B, ihm, iwm),
               "ace: bad shape (B %d, slots of %d x %d; 1..65535 images, sides up to 2^17, at most 2^26 pixels each and 2^31 in all)", B, ihm, iwm);
  VR_CHECK_ARG(radius >= 1 && radius <= ACE_MAXR && bins >= 2 && bins <= ACE_MAXBINS,
               "ace: radius %d must lie in 1..%d and bins %d in 2..%d", radius, ACE_MAXR, bins, ACE_MAXBINS);
  VR_CHECK_ARG(ratio > 0.0 && ratio < __builtin_huge_val() && s >= 0.0 && s < 0.5,
               "ace: ratio %g must be positive and finite and s %g in [0, 0.5)", ratio, s);
  const AceLayout l = ace_layout(B, ihm, iwm);
  if (workspace_bytes < l.total) {
    vr_set_error("ace: the workspace holds %ld bytes, %ld are needed", workspace_bytes, l.total);
    return VR_ERR_WORKSPACE;
  }
  VR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(weights) & 7) == 0,
               "ace: the workspace and the weights must be 8-byte aligned");
  char* ws = static_cast<char*>(workspace);
  AceArgs p;
  p.frames = frames;
  p.geom = geom;
  p.out = out;
  p.flag = flag;
  p.rec = reinterpret_cast<AceRec*>(ws + l.rec);
  p.keys = reinterpret_cast<unsigned long long*>(ws + l.keys);
  p.recd = reinterpret_cast<double*>(ws + l.recd);
  p.hist = reinterpret_cast<int*>(ws + l.hist);
  p.ratio = ratio;
  p.s = s;
  p.ihm = ihm;
  p.iwm = iwm;
  p.bins = bins;
  AceLevel lv[ACE_MAXLEVELS];
  for (int L = 0; L <= l.nl; ++L) {
    lv[L].I = L > 0 ? reinterpret_cast<double*>(ws + l.I[L]) : nullptr;
    lv[L].R = reinterpret_cast<double*>(ws + l.R[L]);
    lv[L].hm = l.hm[L];
    lv[L].wm = l.wm[L];
  }
  hipStream_t st = vr_stream(stream);
  hipLaunchKernelGGL(ace_init_kernel, dim3(B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("ace (init)");
  for (int L = 0; L < l.nl; ++L) {
    const dim3 grid(3 * (unsigned int)vr_cdiv(lv[L + 1].wm, 32), (unsigned int)vr_cdiv(lv[L + 1].hm, 8), B);
    hipLaunchKernelGGL(ace_down_kernel, grid, dim3(256), 0, st, p, lv[L], lv[L + 1], L);
    VR_LAUNCH_CHECK("ace (pyramid)");
  }
  for (int L = l.nl - 1; L >= 0; --L) {
    const dim3 grid(3 * (unsigned int)vr_cdiv(lv[L].wm, ACE_T), (unsigned int)vr_cdiv(lv[L].hm, ACE_T), B);
    switch (radius) {
#define ACE_LEVEL(R_)                                                                                            \
  case R_:                                                                                                       \
    hipLaunchKernelGGL(ace_level_kernel<R_>, grid, dim3(256), 0, st, p, lv[L], lv[L + 1], L, weights);          \
    break;
      ACE_LEVEL(1) ACE_LEVEL(2) ACE_LEVEL(3) ACE_LEVEL(4) ACE_LEVEL(5) ACE_LEVEL(6) ACE_LEVEL(7) ACE_LEVEL(8)
#undef ACE_LEVEL
    }
    VR_LAUNCH_CHECK("ace (level)");
  }
  const dim3 hgrid(3 * (unsigned int)vr_cdiv(iwm, ACE_HW), (unsigned int)vr_cdiv(ihm, ACE_HH), B);
  hipLaunchKernelGGL(ace_hist_kernel, hgrid, dim3(256), 0, st, p, lv[0]);
  VR_LAUNCH_CHECK("ace (histogram)");
  hipLaunchKernelGGL(ace_scan_kernel, dim3(B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("ace (thresholds)");
  const dim3 sgrid((unsigned int)vr_cdiv(iwm, 64), (unsigned int)vr_cdiv(ihm, 4), B);
  hipLaunchKernelGGL(ace_store_kernel, sgrid, dim3(256), 0, st, p, lv[0]);
  VR_LAUNCH_CHECK("ace (stretch)");
  return VR_OK;
}
