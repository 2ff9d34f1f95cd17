// Detection post-processing after the box decode: utils/utils_bbox.py:86-135 `non_max_suppression` and the
// torchvision.ops.boxes.batched_nms it calls (:124).  Four kernels, all deterministic (no result depends on the order in
// which workgroups or waves run):
//   select  one thread per (image, anchor): class max / arg-max over channels 5 .. 5+nc-1 (first index on ties, as
//           torch.max), score = obj * class_conf, kept iff score >= conf (a NaN fails); corner box rows are compacted into
//           a per-image candidate list with a wave ballot and one atomic per wave (list order arbitrary: `order` fixes it)
//   order   rank_i = #{j : key_j precedes key_i}, key = (score descending, id ascending), LDS-tiled; candidates are
//           scattered to their rank.  Ranks are a permutation because the ids of a segment are distinct
//   mask    64 x 64 blocks on or above the diagonal, one wave each: bit j of word (i, j / 64) is set iff j > i, same class
//           and IoU(i, j) > iou_thr (class-aware masks = batched_nms semantics without the coordinate-offset trick)
//   scan    one workgroup per segment, `removed` bit mask in LDS; per 64-row block wave 0 resolves the block serially
//           against its diagonal words (registers), then all waves OR the rows of the kept boxes into the later words;
//           the kept boxes are written out in one parallel pass at the end
// A captured graph needs a fixed candidate capacity: vrnet_nms_capped_f32 runs `order_capped` in place of `order` -- every
// candidate of a segment is ranked, only ranks < cap are scattered, and mask / scan see min(count, cap) boxes.  Greedy NMS
// decides a box from higher-ranked boxes only, so the result is the prefix of the uncapped result: its kept rows of rank
// < cap.  `finish` (vrnet_detect_finish_f32) then restates the host tail of decode.non_max_suppression and render.box_rows
// per kept row: the letterbox un-map in fp64, the integer draw rows with their prefix-sum offsets, the class counts.
// IoU is the torchvision CPU kernel's expression in IEEE fp32 with no contraction (pragma below), compared in
// double: bit-reproducible by a float32 numpy restatement (tests/test_nms.py).
#include "common.h"

// No a*b+c fusion anywhere in this file (hipcc contracts by default, also across the header's __fmul_rn / __fadd_rn): the
// IoU must round after every operation to match the fp32 restatement bit for bit.
#pragma clang fp contract(off)

namespace {

constexpr int NMS_MAX_WORDS = 4096;          // LDS of the scan: 48 KiB, n_max <= 262 144 per segment
constexpr int NMS_FLAG_CANDIDATES = 8;       // bits of the flag word, above render.hip's 1, 2, 4: more candidates than cap
constexpr int NMS_FLAG_DET_CLASS = 16;       // a kept row whose class id lies outside [0, num_classes)

// A 64-bit key whose unsigned order is (score descending, id ascending): the score's bits mapped to an order-preserving
// unsigned integer (-0 folded onto +0 and every NaN onto one value, so equal scores give equal high words), then the id
// inverted so that the lower id compares greater.  A real key is never 0: padding with 0 counts as "not before".
__device__ __forceinline__ unsigned long long nms_key(float s, int id) {
  if (s == 0.0f) s = 0.0f;
  unsigned int u = __float_as_uint(s);
  if (s != s) u = 0x7fc00000u;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned long long)(0xffffffffu - (unsigned int)id);
}

// torchvision/csrc/ops/cpu/nms_kernel.cpp: std::max / std::min argument order kept (it decides which operand a NaN yields)
__device__ __forceinline__ float smax(float a, float b) { return (a < b) ? b : a; }
__device__ __forceinline__ float smin(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float box_area(const float4 b) { return (b.z - b.x) * (b.w - b.y); }

__device__ __forceinline__ bool nms_suppresses(const float4 i, float area_i, const float4 j, double thr) {
  const float w = smax(0.0f, smin(i.z, j.z) - smax(i.x, j.x));
  const float h = smax(0.0f, smin(i.w, j.w) - smax(i.y, j.y));
  const float inter = w * h;
  const float iou = inter / (area_i + box_area(j) - inter);     // IEEE divide: hipcc's default
  return (double)iou > thr;
}

__device__ __forceinline__ unsigned long long lanemask_lt() {
  const int lane = threadIdx.x & 63;
  return lane ? (~0ull >> (64 - lane)) : 0ull;
}

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int lane) {
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, lane);
  const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

struct SelectArgs {
  const float* pred;           // (B, A, C)
  int A, C, nc;
  float conf;
  float* rows;                 // (B, A, 7): x1, y1, x2, y2, obj, class_conf, class_pred
  float* scores;               // (B, A)
  long long* cls;              // (B, A)
  int* ids;                    // (B, A) anchor index
  int* counts;                 // (B) zeroed by the caller
};

__global__ __launch_bounds__(256) void select_kernel(const SelectArgs p) {
  const int b = blockIdx.y, a = blockIdx.x * 256 + threadIdx.x;
  bool keep = false;
  float x1 = 0, y1 = 0, x2 = 0, y2 = 0, obj = 0, best = 0, score = 0;
  int arg = 0;
  if (a < p.A) {
    const float* r = p.pred + ((long)b * p.A + a) * p.C;
    const float cx = r[0], cy = r[1], w = r[2], h = r[3];
    obj = r[4];
    best = r[5];
    bool nan = best != best;
    for (int c = 1; c < p.nc; ++c) {
      const float v = r[5 + c];
      nan |= v != v;
      if (v > best) { best = v; arg = c; }
    }
    // torch.max propagates a NaN, so the score of such a row is NaN and fails the test
    score = obj * best;
    keep = !nan && score >= p.conf;
    x1 = cx - w / 2.0f; y1 = cy - h / 2.0f;
    x2 = cx + w / 2.0f; y2 = cy + h / 2.0f;
  }
  const unsigned long long m = __ballot(keep);
  if (m == 0) return;
  int base = 0;
  if ((threadIdx.x & 63) == 0) base = atomicAdd(p.counts + b, __popcll(m));
  base = __shfl(base, 0);
  if (!keep) return;
  const long o = (long)b * p.A + base + __popcll(m & lanemask_lt());
  float* dst = p.rows + o * 7;
  dst[0] = x1; dst[1] = y1; dst[2] = x2; dst[3] = y2; dst[4] = obj; dst[5] = best; dst[6] = (float)arg;
  p.scores[o] = score;
  p.cls[o] = arg;
  p.ids[o] = a;
}

struct SegArgs {
  const float* rows;           // segment s, element k: box at rows + (s * stride + k) * ld (x1, y1, x2, y2)
  int ld;
  const float* scores;         // scores[s * stride + k]
  const long long* cls;        // cls[s * stride + k]
  const int* ids;              // ids[s * stride + k] or NULL (id = k)
  const int* counts;           // counts[s] or NULL (n_max)
  long stride;
  int n_max, nb;               // nb = 64-row blocks of n_max = words per mask row
  double thr;
  float4* sbox;                // workspace: (S, n_max) each, in rank order
  long long* scls;
  int* spos;                   // rank -> k
  unsigned long long* mask;    // (S, n_max, nb)
  int* keep;                   // (S, n_max): k of the kept boxes in score order
  int* kept;                   // (S)
  float* rows_out;             // (S, n_max, ld) or NULL
  int* flag;                   // order_capped only
};

__device__ __forceinline__ int seg_count(const SegArgs& p, int s) { return p.counts ? min(p.counts[s], p.n_max) : p.n_max; }

__global__ __launch_bounds__(256) void order_kernel(const SegArgs p) {
  __shared__ unsigned long long tile[256];
  const int s = blockIdx.y, n = seg_count(p, s);
  if ((int)blockIdx.x * 256 >= n) return;
  const long off = (long)s * p.stride;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long ki = i < n ? nms_key(p.scores[off + i], p.ids ? p.ids[off + i] : i) : 0;
  int rank = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + threadIdx.x;
    __syncthreads();
    tile[threadIdx.x] = j < n ? nms_key(p.scores[off + j], p.ids ? p.ids[off + j] : j) : 0;
    __syncthreads();
#pragma unroll 16
    for (int t = 0; t < 256; ++t) rank += tile[t] > ki;
  }
  if (i >= n) return;
  const float* r = p.rows + (off + i) * p.ld;
  const long d = (long)s * p.n_max + rank;
  p.sbox[d] = make_float4(r[0], r[1], r[2], r[3]);
  p.scls[d] = p.cls[off + i];
  p.spos[d] = i;
}

// `order` for a fixed capacity n_max = cap: ALL min(counts[s], stride) candidates are ranked, ranks >= cap are dropped (which
// candidates survive does not depend on the arbitrary list order of `select`), and the flag word tells when any were
__global__ __launch_bounds__(256) void order_capped_kernel(const SegArgs p) {
  __shared__ unsigned long long tile[256];
  const int s = blockIdx.y, count = p.counts[s];
  const int n = (int)min((long)max(count, 0), p.stride);
  if ((int)blockIdx.x * 256 >= n) return;
  if (blockIdx.x == 0 && threadIdx.x == 0 && count > p.n_max) atomicOr(p.flag, NMS_FLAG_CANDIDATES);
  const long off = (long)s * p.stride;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long ki = i < n ? nms_key(p.scores[off + i], p.ids ? p.ids[off + i] : i) : 0;
  int rank = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + threadIdx.x;
    __syncthreads();
    tile[threadIdx.x] = j < n ? nms_key(p.scores[off + j], p.ids ? p.ids[off + j] : j) : 0;
    __syncthreads();
#pragma unroll 16
    for (int t = 0; t < 256; ++t) rank += tile[t] > ki;
  }
  if (i >= n || rank >= p.n_max) return;
  const float* r = p.rows + (off + i) * p.ld;
  const long d = (long)s * p.n_max + rank;
  p.sbox[d] = make_float4(r[0], r[1], r[2], r[3]);
  p.scls[d] = p.cls[off + i];
  p.spos[d] = i;
}

__global__ __launch_bounds__(64) void mask_kernel(const SegArgs p) {
  __shared__ float4 rb[64];
  __shared__ long long rc[64];
  const int cb = blockIdx.x, r0 = blockIdx.y * 64, s = blockIdx.z, n = seg_count(p, s);
  if (cb < (int)blockIdx.y || r0 >= n) return;
  const int lane = threadIdx.x, rows = min(64, n - r0);
  const long seg = (long)s * p.n_max;
  if (lane < rows) { rb[lane] = p.sbox[seg + r0 + lane]; rc[lane] = p.scls[seg + r0 + lane]; }
  const int j = cb * 64 + lane;
  float4 bj = make_float4(0, 0, 0, 0);
  long long cj = 0;
  if (j < n) { bj = p.sbox[seg + j]; cj = p.scls[seg + j]; }
  __syncthreads();
  unsigned long long mine = 0;
  for (int t = 0; t < rows; ++t) {
    const float4 bi = rb[t];
    const bool bit = j < n && j > r0 + t && cj == rc[t] && nms_suppresses(bi, box_area(bi), bj, p.thr);
    const unsigned long long w = __ballot(bit);
    if (lane == t) mine = w;
  }
  if (lane < rows) p.mask[(seg + r0 + lane) * p.nb + cb] = mine;
}

// LDS: removed[nb] (after block r is resolved, word r holds its removed rows), base[nb] (kept before block r)
__global__ __launch_bounds__(256) void scan_kernel(const SegArgs p) {
  extern __shared__ unsigned long long removed[];
  __shared__ unsigned long long keep_word;
  __shared__ int keep_rows[64];
  int* base_of = reinterpret_cast<int*>(removed + p.nb);
  const int s = blockIdx.x, n = seg_count(p, s), nbn = (n + 63) / 64;
  const int lane = threadIdx.x & 63;
  const bool wave0 = threadIdx.x < 64;
  const long seg = (long)s * p.n_max;
  const unsigned long long* mask = p.mask + seg * p.nb;
  for (int c = threadIdx.x; c < nbn; c += 256) removed[c] = 0;
  int base = 0;                                       // kept so far (wave 0)
  unsigned long long diag = 0;                        // wave 0: lane t holds word (r * 64 + t, r)
  if (wave0 && lane < n) diag = mask[(long)lane * p.nb];
  for (int r = 0; r < nbn; ++r) {
    __syncthreads();
    if (wave0) {
      const int rows = min(64, n - r * 64);
      const unsigned long long d = diag;
      diag = (r + 1) * 64 + lane < n ? mask[(long)((r + 1) * 64 + lane) * p.nb + r + 1] : 0;   // next block's, early
      unsigned long long cur = removed[r];
      for (int t = 0; t < rows; ++t) {
        const unsigned long long dt = readlane64(d, t);
        cur |= ((cur >> t) & 1) ? 0ull : dt;
      }
      const unsigned long long km = ~cur & (rows == 64 ? ~0ull : ((1ull << rows) - 1));
      if ((km >> lane) & 1) keep_rows[__popcll(km & lanemask_lt())] = lane;
      if (lane == 0) { keep_word = km; removed[r] = cur; base_of[r] = base; }
      base += __popcll(km);
    }
    __syncthreads();
    // OR the later words of the kept rows into `removed`: (kept row, word) pairs spread over the workgroup, eight
    // independent loads in flight per thread
    const int nk = __popcll(keep_word), ncol = nbn - r - 1, tasks = nk * ncol;
    for (int t0 = threadIdx.x; t0 < tasks; t0 += 256 * 8) {
      unsigned long long w[8];
      int col[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = t0 + u * 256, kr = t / max(ncol, 1);
        col[u] = r + 1 + t - kr * ncol;
        w[u] = t < tasks ? mask[(long)(r * 64 + keep_rows[kr]) * p.nb + col[u]] : 0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (w[u]) atomicOr(removed + col[u], w[u]);
    }
  }
  __syncthreads();
  // the kept boxes in score order, all rows in parallel
  for (int i = threadIdx.x; i < n; i += 256) {
    const unsigned long long cur = removed[i >> 6];
    const int bit = i & 63;
    if ((cur >> bit) & 1) continue;
    const int o = base_of[i >> 6] + __popcll(~cur & ((1ull << bit) - 1));
    const int k = p.spos[seg + i];
    p.keep[seg + o] = k;
    if (p.rows_out) {
      const float* src = p.rows + ((long)s * p.stride + k) * p.ld;
      float* dst = p.rows_out + (seg + o) * p.ld;
      for (int c = 0; c < p.ld; ++c) dst[c] = src[c];
    }
  }
  if (threadIdx.x == 0) p.kept[s] = base;
}

struct FinishArgs {
  const float* rows;           // (B, cap, 7) kept rows: x1, y1, x2, y2 of the network input, obj, class_conf, class
  const int* kept;             // (B)
  int B, cap, nc, ih, iw;
  double off_y, off_x, sc_y, sc_x, img_h, img_w;
  float* out;                  // (B, cap, 7): top, left, bottom, right in pixels of the original image, obj, class_conf, class
  int* draw;                   // (B * cap, 5) zeroed by the caller: left, top, right, bottom, class, the images back to back
  int* offsets;                // (B + 1)
  unsigned long long* counts;  // (B, nc) zeroed by the caller
  int* flag;
  const vrnet_frame_geom* tab; // RAGGED only: (B) records; ih, iw and the four scalars of image b come from tab[b],
  int ihm, iwm;                // clamped to the slot ihm x iwm
};

// np.clip(np.floor(float64(v)), -2^31, 2^31 - 1).astype(int64) of render.box_rows
__device__ __forceinline__ int floor_clip(float v) {
  double f = floor((double)v);
  f = f < -2147483648.0 ? -2147483648.0 : (f > 2147483647.0 ? 2147483647.0 : f);
  return (int)f;
}

// One thread per (image, row slot).  The fp32 centre / size of decode.non_max_suppression, then decode.yolo_correct_boxes
// in fp64 operation by operation (no contraction: the pragma above), one rounding to fp32 as the assignment into the
// float32 array does; without a letterbox the caller passes offset 0 and scale 1, which change no bit.
template <bool RAGGED>
__global__ __launch_bounds__(256) void detect_finish_kernel(const FinishArgs p) {
  __shared__ int part[256];
  const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  int ih = p.ih, iw = p.iw;
  double off_y = p.off_y, off_x = p.off_x, sc_y = p.sc_y, sc_x = p.sc_x, img_h = p.img_h, img_w = p.img_w;
  if constexpr (RAGGED) {                             // the image's own record: the block's, so wave-uniform
    bool bad;
    const vrnet_frame_geom g = vr_geom_load(p.tab, b, p.ihm, p.iwm, 0, 0, bad);
    if (bad && k == 0) atomicOr(p.flag, VR_FLAG_GEOMETRY);
    ih = g.ih; iw = g.iw;
    off_y = g.offset_y; off_x = g.offset_x; sc_y = g.scale_y; sc_x = g.scale_x;
    img_h = (double)g.ih; img_w = (double)g.iw;
  }
  int before = 0;                                     // kept rows of the images in front of this one
  for (int j = threadIdx.x; j < b; j += 256) before += min(max(p.kept[j], 0), p.cap);
  part[threadIdx.x] = before;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  const int base = part[0], n = min(max(p.kept[b], 0), p.cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (b == 0) p.offsets[0] = 0;
    p.offsets[b + 1] = base + n;
  }
  if (k >= p.cap) return;
  const float* r = p.rows + ((long)b * p.cap + k) * 7;
  float* o = p.out + ((long)b * p.cap + k) * 7;
  if (k >= n) {
    for (int c = 0; c < 7; ++c) o[c] = 0.0f;
    return;
  }
  const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
  const float cx = (x1 + x2) / 2.0f, cy = (y1 + y2) / 2.0f, w = x2 - x1, h = y2 - y1;
  double c_y = (double)cy, c_x = (double)cx, s_y = (double)h, s_x = (double)w;
  c_y = (c_y - off_y) * sc_y;
  c_x = (c_x - off_x) * sc_x;
  s_y = s_y * sc_y;
  s_x = s_x * sc_x;
  const double hy = 0.5 * s_y, hx = 0.5 * s_x;
  const float top = (float)((c_y - hy) * img_h), left = (float)((c_x - hx) * img_w);
  const float bottom = (float)((c_y + hy) * img_h), right = (float)((c_x + hx) * img_w);
  o[0] = top; o[1] = left; o[2] = bottom; o[3] = right; o[4] = r[4]; o[5] = r[5]; o[6] = r[6];
  const int label = (int)r[6];
  int* d = p.draw + 5L * (base + k);
  d[0] = max(0, floor_clip(left));
  d[1] = max(0, floor_clip(top));
  d[2] = min(iw, floor_clip(right));
  d[3] = min(ih, floor_clip(bottom));
  d[4] = label;
  if (label >= 0 && label < p.nc) atomicAdd(p.counts + (long)b * p.nc + label, 1ull);
  else atomicOr(p.flag, NMS_FLAG_DET_CLASS);
}

long seg_mask_words(long n_max) { return n_max * vr_cdiv(n_max, 64); }

}  // namespace

extern "C" int vrnet_detect_select_f32(const float* pred, int B, int A, int C, int num_classes, float conf_thres,
                                       float* rows, float* scores, long long* cls, int* ids, int* counts, void* stream) {
  VR_CHECK_ARG(pred && rows && scores && cls && ids && counts && B > 0 && A > 0 && num_classes >= 1 && 5 + num_classes <= C,
               "detect_select: bad arguments (B, A > 0, 1 <= num_classes <= C - 5)");
  VR_CHECK_ARG((long)B * A < (1L << 31) && B < 65536, "detect_select: too many anchors");
  if (hipMemsetAsync(counts, 0, sizeof(int) * B, vr_stream(stream)) != hipSuccess) {
    vr_set_error("detect_select: memset failed");
    return VR_ERR_LAUNCH;
  }
  SelectArgs p{pred, A, C, num_classes, conf_thres, rows, scores, cls, ids, counts};
  hipLaunchKernelGGL(select_kernel, dim3(vr_cdiv(A, 256), B), dim3(256), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK("detect_select");
  return VR_OK;
}

extern "C" long vrnet_nms_workspace_bytes(int segments, int n_max) {
  if (segments <= 0 || n_max <= 0) return 0;
  const long per = seg_mask_words(n_max) * 8 + (long)n_max * (sizeof(float4) + sizeof(long long) + sizeof(int));
  return segments * per + 256;
}

// the three launches of both NMS entry points; `flag` non-NULL selects the capped order
static int nms_run(const char* fn, const float* rows, int ld, const float* scores, const long long* classes, const int* ids,
                   const int* counts, int segments, long stride, int n_max, double iou_thres, void* workspace,
                   long workspace_bytes, int* keep, int* kept, float* rows_out, int* flag, void* stream) {
  VR_CHECK_ARG(rows && scores && classes && keep && kept && segments > 0 && segments < 65536 && n_max > 0 && ld >= 4 &&
                   stride >= n_max, "%s: bad arguments", fn);
  VR_CHECK_ARG(vr_cdiv(n_max, 64) <= NMS_MAX_WORDS, "%s: n_max %d above %d", fn, n_max, NMS_MAX_WORDS * 64);
  VR_CHECK_ARG(workspace && workspace_bytes >= vrnet_nms_workspace_bytes(segments, n_max), "%s: workspace %ld < %ld", fn,
               workspace_bytes, vrnet_nms_workspace_bytes(segments, n_max));
  const long SN = (long)segments * n_max;
  SegArgs p{};
  p.rows = rows; p.ld = ld; p.scores = scores; p.cls = classes; p.ids = ids; p.counts = counts;
  p.stride = stride; p.n_max = n_max; p.nb = (int)vr_cdiv(n_max, 64); p.thr = iou_thres;
  char* w = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t(255));
  p.sbox = reinterpret_cast<float4*>(w);               w += SN * sizeof(float4);
  p.mask = reinterpret_cast<unsigned long long*>(w);   w += segments * seg_mask_words(n_max) * 8;
  p.scls = reinterpret_cast<long long*>(w);            w += SN * sizeof(long long);
  p.spos = reinterpret_cast<int*>(w);
  p.keep = keep; p.kept = kept; p.rows_out = rows_out; p.flag = flag;
  const hipStream_t st = vr_stream(stream);
  if (flag)
    hipLaunchKernelGGL(order_capped_kernel, dim3(vr_cdiv(stride, 256), segments), dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL(order_kernel, dim3(vr_cdiv(n_max, 256), segments), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("nms order");
  hipLaunchKernelGGL(mask_kernel, dim3(p.nb, p.nb, segments), dim3(64), 0, st, p);
  VR_LAUNCH_CHECK("nms mask");
  hipLaunchKernelGGL(scan_kernel, dim3(segments), dim3(256), p.nb * (sizeof(unsigned long long) + sizeof(int)), st, p);
  VR_LAUNCH_CHECK("nms scan");
  return VR_OK;
}

extern "C" int vrnet_nms_segmented_f32(const float* rows, int ld, const float* scores, const long long* classes,
                                       const int* ids, const int* counts, int segments, long stride, int n_max,
                                       double iou_thres, void* workspace, long workspace_bytes, int* keep, int* kept,
                                       float* rows_out, void* stream) {
  return nms_run("nms_segmented", rows, ld, scores, classes, ids, counts, segments, stride, n_max, iou_thres, workspace,
                 workspace_bytes, keep, kept, rows_out, nullptr, stream);
}

extern "C" int vrnet_nms_capped_f32(const float* rows, int ld, const float* scores, const long long* classes, const int* ids,
                                    const int* counts, int segments, long stride, int cap, double iou_thres, void* workspace,
                                    long workspace_bytes, int* keep, int* kept, float* rows_out, int* flag, void* stream) {
  VR_CHECK_ARG(counts && flag && stride > 0 && stride < (1L << 31), "nms_capped: needs device counts, a flag word and stride < 2^31");
  return nms_run("nms_capped", rows, ld, scores, classes, ids, counts, segments, stride, cap, iou_thres, workspace,
                 workspace_bytes, keep, kept, rows_out, flag, stream);
}

// the checks, the clears and the launch of both detect_finish entry points, on `p` as the entry point filled it; `what`
// names the size h x w in the message
static int finish_run(const char* fn, bool ragged, const char* what, int h, int w, const FinishArgs& p, void* stream) {
  VR_CHECK_ARG(p.rows && p.kept && (p.tab || !ragged) && p.out && p.draw && p.offsets && p.counts && p.flag && p.rows != p.out,
               "%s: every array is required, rows_out apart from rows", fn);
  VR_CHECK_ARG(p.B > 0 && p.B < 65536 && p.cap > 0 && (long)p.B * p.cap < (1L << 27) && p.nc >= 1 && h > 0 && w > 0,
               "%s: bad shape (B %d, cap %d, %d classes, %s %d x %d)", fn, p.B, p.cap, p.nc, what, h, w);
  const hipStream_t st = vr_stream(stream);
  if (hipMemsetAsync(p.draw, 0, sizeof(int) * 5 * (size_t)p.B * p.cap, st) != hipSuccess ||
      hipMemsetAsync(p.counts, 0, sizeof(long long) * (size_t)p.B * p.nc, st) != hipSuccess) {
    vr_set_error("%s: memset failed", fn);
    return VR_ERR_LAUNCH;
  }
  if (ragged) hipLaunchKernelGGL(detect_finish_kernel<true>, dim3(vr_cdiv(p.cap, 256), p.B), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(detect_finish_kernel<false>, dim3(vr_cdiv(p.cap, 256), p.B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK(fn);
  return VR_OK;
}

extern "C" int vrnet_detect_finish_f32(const float* rows, const int* kept, int B, int cap, int num_classes, int image_h,
                                       int image_w, double offset_y, double offset_x, double scale_y, double scale_x,
                                       float* rows_out, int* draw_rows, int* offsets, long long* det_counts, int* flag,
                                       void* stream) {
  FinishArgs p{};
  p.rows = rows; p.kept = kept; p.B = B; p.cap = cap; p.nc = num_classes; p.ih = image_h; p.iw = image_w;
  p.off_y = offset_y; p.off_x = offset_x; p.sc_y = scale_y; p.sc_x = scale_x; p.img_h = (double)image_h; p.img_w = (double)image_w;
  p.out = rows_out; p.draw = draw_rows; p.offsets = offsets; p.counts = reinterpret_cast<unsigned long long*>(det_counts);
  p.flag = flag;
  return finish_run("detect_finish", false, "image", image_h, image_w, p, stream);
}

extern "C" int vrnet_detect_finish_ragged_f32(const float* rows, const int* kept, const vrnet_frame_geom* geom, int B, int cap,
                                              int num_classes, int ihm, int iwm, float* rows_out, int* draw_rows, int* offsets,
                                              long long* det_counts, int* flag, void* stream) {
  FinishArgs p{};
  p.rows = rows; p.kept = kept; p.B = B; p.cap = cap; p.nc = num_classes; p.tab = geom; p.ihm = ihm; p.iwm = iwm;
  p.out = rows_out; p.draw = draw_rows; p.offsets = offsets; p.counts = reinterpret_cast<unsigned long long*>(det_counts);
  p.flag = flag;
  return finish_run("detect_finish_ragged", true, "slots", ihm, iwm, p, stream);
}
