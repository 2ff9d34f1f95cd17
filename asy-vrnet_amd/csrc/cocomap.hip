// The COCO detection metric the evaluation callback logs: utils/utils_map.py:894-923 `get_coco_map` (called at
// utils/callbacks.py:224), i.e. COCOeval(cocoGt, cocoDt, 'bbox') with evaluate(), accumulate(), summarize() on what
// preprocess_gt / preprocess_dr (:800-892) hand it.  Ten IoU thresholds x four area ranges x three per-image detection caps,
// a 101-point precision envelope, twelve summary numbers.  The host (metrics.coco_map) sorts and groups in torch, as it does
// for csrc/detmap.hip; four kernels, all deterministic (integer atomics only, no result depends on the order in which
// workgroups or waves run):
//   counts     one thread per ground truth: npig[class][range] += 1 unless it is a crowd or its area lies outside the range
//   match      one wave per (image, class) group that has a detection, from a compact group list.  The IoU of every
//              (detection, ground truth) pair of the group is computed once, then lanes 0..39 each run the greedy walk of one
//              (threshold, range) pair over the detections in score order with a matched bit set of their own.  "Non-ignored
//              ground truths first, stably" is two passes over the input order, the second only if the first found nothing
//              (the walk stops at the first ignored ground truth once it holds a non-ignored one).  IoUs, bit sets and flags
//              live in LDS when they fit 64 KiB, otherwise in the group's slice of the workspace.
//   curve      one workgroup per (class, threshold, range), over the class's detections in (score, image, rank) order with
//              the three caps M side by side, masked by "rank inside its group < M" (a masked or ignored entry adds nothing
//              and repeats its predecessor's recall and precision, so it changes neither the envelope nor a look-up).  Pass
//              1 packs a byte per detection and reduces the tp / fp totals; pass 2 walks the chunks from the back: suffix
//              sums with a carry (wave scans through __shfl_down) give the cumulative tp / fp of every position, the suffix
//              maximum of the precision is the envelope, and a true positive that raises the count to v writes the envelope
//              to every recall point whose smallest sufficient count is v (a binary search over the 101 counts, themselves
//              found by binary search: tp / npig is monotone in tp)
//   summarise  one workgroup per summary number: per-thread strided sums in index order, then a fixed tree
// Every decision is IEEE fp64 with one rounding per operation (pragma below) in COCOeval's operand order, so a Python-float
// restatement reproduces matches, precision and recall bit for bit (tests/test_cocomap.py).
#include "common.h"

// No a*b+c fusion anywhere in this file: IoU, recall and precision must round after every operation, as Python's floats.
#pragma clang fp contract(off)

namespace {

constexpr int CM_T = 10, CM_A = 4, CM_M = 3, CM_R = 101;
constexpr int CM_CH = CM_T * CM_A;           // the chains of a group: (threshold, range) pairs, chain = t * 4 + a
constexpr int CM_MAXDET = 100;               // maxDets[-1]: detections kept per (image, class)
constexpr int CM_MAX_N = 1 << 24;
constexpr int CM_MAX_CLASSES = 65535;
constexpr int CM_LDS = 65536;
constexpr int CM_BLOCK = 512, CM_WAVES = CM_BLOCK / 64;
constexpr int CM_SUM_BLOCK = 1024;
constexpr int CM_COUNT_LDS = 2048;

struct CocoArgs {
  const double* det_box;         // (D, 4) input order: left, top, right, bottom
  const int* order;              // (D) slot -> input index: grouped by (image, class), score descending, ties in input order
  const int* rank;               // (D) by slot: position inside its group
  const int* cslot;              // (D) class order -> slot: classes ascending, score descending, ties by image then rank
  const int* det_off;            // (C + 1) class order positions of class c
  int D;
  const int* grp_start;          // (NG + 1) slots of group k
  const int* grp_gt;             // (NG, 2) the group's range in gt_perm
  const long* grp_ws;            // (NG) byte offset of the group's workspace slice (groups that do not fit LDS)
  int lds_bytes;
  const double* gt_box;          // (G, 4) input order
  const double* gt_area;         // (G)
  const unsigned char* gt_crowd; // (G)
  const int* gt_label;           // (G)
  const int* gt_perm;            // (G) grouped by (image, class), input order inside a group
  int G, C, zero_id;
  const double* thr;             // (10) device
  const double* rec;             // (101) device
  int* match;                    // (40, D) by slot
  unsigned char* code;           // (40, D) by slot: 0 fp, 1 tp, 2 ignored, 3 cut by the 100 per group
  int* n_gt;                     // (C, 4)
  double* precision;             // (10, 101, C, 4, 3)
  double* recall;                // (10, C, 4, 3)
  double* stats;                 // (12)
  unsigned char* pack;           // workspace (40, D) by class order: the curve kernel's byte per detection
  unsigned char* slices;         // workspace: the groups' slices
  long slice_bytes;
};

// areaRng: all [0, 1e5^2], small [0, 32^2], medium [32^2, 96^2], large [96^2, 1e5^2]
__device__ __forceinline__ bool cm_outside(double area, int a) {
  const double lo = a == 2 ? 1024.0 : (a == 3 ? 9216.0 : 0.0);
  const double hi = a == 1 ? 1024.0 : (a == 2 ? 9216.0 : 1e10);
  return area < lo || area > hi;
}

__host__ __device__ inline long cm_group_bytes(long Dg, long Gg) {
  return 8 * Dg * Gg + 4 * CM_CH * ((Gg + 31) >> 5) + ((Gg + 7) & ~7L);
}

__global__ __launch_bounds__(256) void cm_counts_kernel(const CocoArgs p) {
  __shared__ int hist[CM_COUNT_LDS];             // up to 512 classes: the block's counts first, one global atomic per counter
  const int g = blockIdx.x * 256 + threadIdx.x, nbin = p.C * CM_A;
  const bool local = nbin <= CM_COUNT_LDS;
  if (local) {
    for (int i = threadIdx.x; i < nbin; i += 256) hist[i] = 0;
    __syncthreads();
  }
  if (g < p.G) {
    const int c = p.gt_label[g];
    if (c >= 0 && c < p.C && !p.gt_crowd[g]) {
      const double area = p.gt_area[g];
#pragma unroll
      for (int a = 0; a < CM_A; ++a)
        if (!cm_outside(area, a)) atomicAdd((local ? hist : p.n_gt) + c * CM_A + a, 1);
    }
  }
  if (local) {
    __syncthreads();
    for (int i = threadIdx.x; i < nbin; i += 256)
      if (hist[i]) atomicAdd(p.n_gt + i, hist[i]);
  }
}

__global__ __launch_bounds__(64) void cm_match_kernel(const CocoArgs p) {
  extern __shared__ double cm_smem[];
  const int gi = blockIdx.x, lane = threadIdx.x;
  // the host's tables are clamped so that no access derived from them leaves an array
  const int s0 = vr_clampi(p.grp_start[gi], 0, p.D), s1 = vr_clampi(p.grp_start[gi + 1], s0, p.D);
  const int cnt = s1 - s0, Dg = min(cnt, CM_MAXDET);
  const int glo = vr_clampi(p.grp_gt[2 * gi], 0, p.G), Gg = vr_clampi(p.grp_gt[2 * gi + 1], glo, p.G) - glo;
  const long iou_b = 8L * Dg * Gg, gtm_b = 4L * CM_CH * ((Gg + 31) >> 5), need = cm_group_bytes(Dg, Gg);
  unsigned char* base = reinterpret_cast<unsigned char*>(cm_smem);
  int first_cut = Dg;
  if (need > p.lds_bytes) {
    const long off = p.grp_ws[gi];
    if (off < 0 || (off & 7) || off + need > p.slice_bytes) first_cut = 0;   // never with the host's offsets: nothing is matched
    else base = p.slices + off;
  }
  for (long i = lane; i < (long)(cnt - first_cut) * CM_CH; i += 64) {
    const long o = (i % CM_CH) * p.D + s0 + first_cut + i / CM_CH;
    p.match[o] = -1;
    p.code[o] = 3;
  }
  if (first_cut == 0) return;
  double* iou = reinterpret_cast<double*>(base);
  unsigned* gtm = reinterpret_cast<unsigned*>(base + iou_b);       // word w of chain c at gtm[w * 40 + c]
  unsigned char* gf = base + iou_b + gtm_b;                         // bit a: ignored in range a; bit 4: crowd
  for (int g = lane; g < Gg; g += 64) {
    const int gin = p.gt_perm[glo + g];
    const double area = p.gt_area[gin];
    unsigned f = p.gt_crowd[gin] ? 0x1fu : 0u;
#pragma unroll
    for (int a = 0; a < CM_A; ++a) f |= cm_outside(area, a) ? (1u << a) : 0u;
    gf[g] = (unsigned char)f;
  }
  for (int i = lane; i < CM_CH * ((Gg + 31) >> 5); i += 64) gtm[i] = 0;
  for (int i = lane; i < Dg * Gg; i += 64) {
    const int d = i / Gg, g = i - d * Gg;
    const double* db = p.det_box + 4L * p.order[s0 + d];
    const int gin = p.gt_perm[glo + g];
    const double* gb = p.gt_box + 4L * gin;
    const double dx = db[0], dy = db[1], dw = db[2] - db[0], dh = db[3] - db[1];
    const double gx = gb[0], gy = gb[1], gw = gb[2] - gb[0], gh = gb[3] - gb[1];
    const double r0 = dx + dw, r1 = gx + gw, b0 = dy + dh, b1 = gy + gh;
    const double w = (r1 < r0 ? r1 : r0) - (gx > dx ? gx : dx);
    double v = 0.0;
    if (w > 0.0) {
      const double h = (b1 < b0 ? b1 : b0) - (gy > dy ? gy : dy);
      if (h > 0.0) {
        const double in = w * h;
        const double un = p.gt_crowd[gin] ? dw * dh : dw * dh + gw * gh - in;
        v = in / un;
      }
    }
    iou[i] = v;
  }
  __syncthreads();
  if (lane >= CM_CH) return;
  const int a = lane & 3;
  const double t0 = p.thr[lane >> 2], cap = 1.0 - 1e-10, start = cap < t0 ? cap : t0;
  for (int d = 0; d < Dg; ++d) {
    const double* db = p.det_box + 4L * p.order[s0 + d];
    const bool aout = cm_outside((db[2] - db[0]) * (db[3] - db[1]), a);
    const double* row = iou + (long)d * Gg;
    double best = start;
    int m = -1;
    for (int g = 0; g < Gg; ++g) {                                  // the ground truths not ignored in this range
      if ((gf[g] >> a) & 1) continue;
      if ((gtm[(g >> 5) * CM_CH + lane] >> (g & 31)) & 1) continue;
      const double v = row[g];
      if (v < best) continue;
      best = v;
      m = g;
    }
    if (m < 0)
      for (int g = 0; g < Gg; ++g) {                                // then the ignored ones; a crowd may be matched again
        const unsigned f = gf[g];
        if (!((f >> a) & 1)) continue;
        if (((gtm[(g >> 5) * CM_CH + lane] >> (g & 31)) & 1) && !(f & 16)) continue;
        const double v = row[g];
        if (v < best) continue;
        best = v;
        m = g;
      }
    int gm = -1;
    unsigned char code;
    if (m >= 0) {
      gtm[(m >> 5) * CM_CH + lane] |= 1u << (m & 31);
      gm = p.gt_perm[glo + m];
      // annotation id 0 (zero_id): the ground truth is consumed but dtm == 0 reads as "unmatched"
      const bool counted = gm != p.zero_id, ign = ((gf[m] >> a) & 1) || (!counted && aout);
      code = ign ? 2 : (counted ? 1 : 0);
    } else {
      code = aout ? 2 : 0;
    }
    p.match[(long)lane * p.D + s0 + d] = gm;
    p.code[(long)lane * p.D + s0 + d] = code;
  }
}

__global__ __launch_bounds__(CM_BLOCK) void cm_curve_kernel(const CocoArgs p) {
  __shared__ int wsum[CM_WAVES][2 * CM_M], tot[2 * CM_M], need[CM_R];
  __shared__ double wmax[CM_WAVES][CM_M];
  const int c = blockIdx.x, ch = blockIdx.y, t = ch >> 2, a = ch & 3, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lo = p.det_off[c], n = p.det_off[c + 1] - lo;
  const int npig = p.n_gt[c * CM_A + a];
  unsigned char* pk = p.pack + (long)ch * p.D + lo;
  double* prec = p.precision + (((long)t * CM_R * p.C + c) * CM_A + a) * CM_M;     // + r * C * 12 + m
  double* rcl = p.recall + (((long)t * p.C + c) * CM_A + a) * CM_M;
  const long rstride = (long)p.C * CM_A * CM_M;
  if (npig <= 0 || n <= 0) {
    const double v = npig <= 0 ? -1.0 : 0.0;       // no ground truth: the class stays -1; no detection: recall and precision 0
    if (tid < CM_R)
      for (int m = 0; m < CM_M; ++m) prec[tid * rstride + m] = v;
    if (tid < CM_M) rcl[tid] = v;
    return;
  }
  const double dn = (double)npig, eps = 0x1.0p-52;
  // np.searchsorted(rc, recThrs, side='left') finds the first index whose recall tp / npig reaches the point: with the
  // division monotone in tp that is the first index whose cumulative tp reaches need[r], the smallest such count
  if (tid < CM_R) {
    const double want = p.rec[tid];
    int l = 0, h = npig;
    while (l < h) {
      const int mid = (l + h) >> 1;
      if ((double)mid / dn >= want) h = mid;
      else l = mid + 1;
    }
    need[tid] = l;
  }
  // pass 1, in class order: one byte per detection -- bits 0-1: how many of the caps 100, 10, 1 its rank passes, bit 2: a
  // true positive, bit 3: a false positive (neither: ignored) -- and the totals per cap
  int cnt[2 * CM_M] = {0, 0, 0, 0, 0, 0};
  for (int i = tid; i < n; i += CM_BLOCK) {
    const int s = p.cslot[lo + i], rk = p.rank[s], cd = p.code[(long)ch * p.D + s];
    const int level = rk < 1 ? 3 : (rk < 10 ? 2 : (rk < CM_MAXDET ? 1 : 0));
    pk[i] = (unsigned char)(level | (cd == 1 ? 4 : 0) | (cd == 0 ? 8 : 0));
#pragma unroll
    for (int m = 0; m < CM_M; ++m) {
      cnt[2 * m] += (level >= CM_M - m) && cd == 1;
      cnt[2 * m + 1] += (level >= CM_M - m) && cd == 0;
    }
  }
#pragma unroll
  for (int k = 0; k < 2 * CM_M; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt[k] += __shfl_xor(cnt[k], off, 64);
    if (lane == 0) wsum[wv][k] = cnt[k];
  }
  __syncthreads();
  if (tid < 2 * CM_M) {
    int v = 0;
    for (int w = 0; w < CM_WAVES; ++w) v += wsum[w][tid];
    tot[tid] = v;
  }
  __syncthreads();
  int total[2 * CM_M];
#pragma unroll
  for (int k = 0; k < 2 * CM_M; ++k) total[k] = tot[k];
  // a recall point no prefix reaches: precision 0
  if (tid < CM_R)
    for (int m = 0; m < CM_M; ++m)
      if (need[tid] > tot[2 * m]) prec[tid * rstride + m] = 0.0;
  // pass 2, from the back, the three caps side by side: suffix sums give the cumulative tp / fp of every position
  // (cumulative = total - suffix + own), from them the precision; its suffix maximum is the envelope; a true positive
  // that brings the count to v answers every recall point with need[r] == v
  int later[2 * CM_M] = {0, 0, 0, 0, 0, 0};
  double envc[CM_M] = {0.0, 0.0, 0.0};
  for (int base = (n - 1) / CM_BLOCK * CM_BLOCK; base >= 0; base -= CM_BLOCK) {
    const int i = base + tid;
    const bool v = i < n;
    const int b = v ? pk[i] : 0, level = b & 3;
    int own[2 * CM_M], suf[2 * CM_M];
#pragma unroll
    for (int m = 0; m < CM_M; ++m) {
      own[2 * m] = (level >= CM_M - m) && (b & 4);
      own[2 * m + 1] = (level >= CM_M - m) && (b & 8);
    }
#pragma unroll
    for (int k = 0; k < 2 * CM_M; ++k) {
      int x = own[k];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_down(x, off, 64);
        if (lane + off < 64) x += u;
      }
      suf[k] = x;
      if (lane == 0) wsum[wv][k] = x;
    }
    __syncthreads();
    double q[CM_M];
    int ctp[CM_M];
#pragma unroll
    for (int m = 0; m < CM_M; ++m) {
      int sx = later[2 * m] + suf[2 * m], sy = later[2 * m + 1] + suf[2 * m + 1];
#pragma unroll
      for (int w = 0; w < CM_WAVES; ++w) {
        const int x = wsum[w][2 * m], y = wsum[w][2 * m + 1];
        if (w > wv) { sx += x; sy += y; }
        later[2 * m] += x; later[2 * m + 1] += y;
      }
      ctp[m] = total[2 * m] - sx + own[2 * m];
      const int cfp = total[2 * m + 1] - sy + own[2 * m + 1];
      double e = v ? (double)ctp[m] / (((double)cfp + (double)ctp[m]) + eps) : 0.0;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const double u = __shfl_down(e, off, 64);
        if (lane + off < 64 && u > e) e = u;
      }
      q[m] = e;
      if (lane == 0) wmax[wv][m] = e;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < CM_M; ++m) {
      double after = envc[m];
#pragma unroll
      for (int w = 0; w < CM_WAVES; ++w) {
        const double x = wmax[w][m];
        if (w > wv && x > after) after = x;
        if (x > envc[m]) envc[m] = x;
      }
      if (after > q[m]) q[m] = after;
      if (own[2 * m]) {
        int l = 0, h = CM_R;                     // the first r with need[r] >= ctp; need is non-decreasing in r
        while (l < h) {
          const int mid = (l + h) >> 1;
          if (need[mid] >= ctp[m]) h = mid;
          else l = mid + 1;
        }
        for (int r = l; r < CM_R && need[r] == ctp[m]; ++r) prec[r * rstride + m] = q[m];
      }
    }
    __syncthreads();
  }
  // need[r] == 0 (recall point 0): index 0, whose envelope is the maximum of them all
  if (tid < CM_R && need[tid] == 0)
    for (int m = 0; m < CM_M; ++m) prec[tid * rstride + m] = envc[m];
  if (tid < CM_M) rcl[tid] = (double)tot[2 * tid] / dn;
}

__global__ __launch_bounds__(CM_SUM_BLOCK) void cm_summarise_kernel(const CocoArgs p) {
  __shared__ double ssum[CM_SUM_BLOCK];
  __shared__ int scnt[CM_SUM_BLOCK];
  const int s = blockIdx.x, tid = threadIdx.x;
  // COCOeval.summarize: AP over all thresholds, at 0.5, at 0.75 (all areas, 100 detections), AP small / medium / large,
  // AR at 1 / 10 / 100 detections, AR small / medium / large
  const bool ap = s < 6;
  const int t0 = s == 1 ? 0 : (s == 2 ? 5 : 0), nt = (s == 1 || s == 2) ? 1 : CM_T;
  const int a = ap ? (s >= 3 ? s - 2 : 0) : (s >= 9 ? s - 8 : 0);
  const int m = (s == 6) ? 0 : (s == 7 ? 1 : 2);
  const long per_t = ap ? (long)CM_R * p.C : p.C, n = nt * per_t;
  double sum = 0.0;
  int cnt = 0;
  for (long i = tid; i < n; i += CM_SUM_BLOCK) {
    const long tt = t0 + i / per_t, rc = i % per_t;                 // rc = r * C + c, or c
    const double v = ap ? p.precision[((tt * CM_R * p.C + rc) * CM_A + a) * CM_M + m]
                        : p.recall[((tt * p.C + rc) * CM_A + a) * CM_M + m];
    if (v > -1.0) { sum += v; ++cnt; }
  }
  ssum[tid] = sum;
  scnt[tid] = cnt;
  __syncthreads();
  for (int h = CM_SUM_BLOCK / 2; h > 0; h >>= 1) {
    if (tid < h) { ssum[tid] += ssum[tid + h]; scnt[tid] += scnt[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) p.stats[s] = scnt[0] ? ssum[0] / (double)scnt[0] : -1.0;
}

}  // namespace

extern "C" long vrnet_coco_map_group_bytes(int n_det, int n_gt) {
  if (n_det < 0 || n_gt < 0) return 0;
  return cm_group_bytes(n_det < CM_MAXDET ? n_det : CM_MAXDET, n_gt);
}

extern "C" long vrnet_coco_map_workspace_bytes(int D, long slice_bytes) {
  if (D < 0 || slice_bytes < 0) return 0;
  return 256 + vr_align256((long)CM_CH * D) + vr_align256(slice_bytes);
}

extern "C" int vrnet_coco_map_f64(const double* det_box, const int* order, const int* rank, const int* class_slot,
                                  const int* det_offsets, int D, const int* group_start, const int* group_gt,
                                  const long* group_ws, int n_groups, int lds_bytes, long slice_bytes, const double* gt_box,
                                  const double* gt_area, const unsigned char* gt_crowd, const int* gt_label,
                                  const int* gt_perm, int G, int num_classes, int zero_id_gt, const double* iou_thrs,
                                  const double* rec_thrs, int* dt_match, unsigned char* dt_code, int* n_gt, double* precision,
                                  double* recall, double* stats, void* workspace, long workspace_bytes, void* stream) {
  VR_CHECK_ARG(D >= 0 && D <= CM_MAX_N && G >= 0 && G <= CM_MAX_N, "coco_map: %d detections, %d ground truths (0..%d each)", D,
               G, CM_MAX_N);
  VR_CHECK_ARG(num_classes >= 1 && num_classes <= CM_MAX_CLASSES, "coco_map: %d classes (1..%d supported)", num_classes,
               CM_MAX_CLASSES);
  VR_CHECK_ARG(n_groups >= 0 && n_groups <= D && (D == 0) == (n_groups == 0), "coco_map: %d groups for %d detections", n_groups, D);
  VR_CHECK_ARG(lds_bytes >= 0 && lds_bytes <= CM_LDS && slice_bytes >= 0 && slice_bytes % 8 == 0,
               "coco_map: %d bytes of LDS (0..%d), %ld bytes of slices (a multiple of 8)", lds_bytes, CM_LDS, slice_bytes);
  VR_CHECK_ARG(zero_id_gt >= -1 && zero_id_gt < G,
               "coco_map: zero_id_gt %d outside the %d ground truths (-1: none)", zero_id_gt, G);
  VR_CHECK_ARG(det_offsets && iou_thrs && rec_thrs && n_gt && precision && recall && stats &&
                   (D == 0 || (det_box && order && rank && class_slot && group_start && group_gt && group_ws && dt_match && dt_code)) &&
                   (G == 0 || (gt_box && gt_area && gt_crowd && gt_label && gt_perm)),
               "coco_map: missing argument");
  if (!workspace || workspace_bytes < vrnet_coco_map_workspace_bytes(D, slice_bytes)) {
    vr_set_error("coco_map: workspace %ld < %ld bytes", workspace_bytes, vrnet_coco_map_workspace_bytes(D, slice_bytes));
    return VR_ERR_WORKSPACE;
  }
  CocoArgs p{};
  p.det_box = det_box; p.order = order; p.rank = rank; p.cslot = class_slot; p.det_off = det_offsets; p.D = D;
  p.grp_start = group_start; p.grp_gt = group_gt; p.grp_ws = group_ws; p.lds_bytes = lds_bytes;
  p.gt_box = gt_box; p.gt_area = gt_area; p.gt_crowd = gt_crowd; p.gt_label = gt_label; p.gt_perm = gt_perm;
  p.G = G; p.C = num_classes; p.zero_id = zero_id_gt;
  p.thr = iou_thrs; p.rec = rec_thrs;
  p.match = dt_match; p.code = dt_code; p.n_gt = n_gt; p.precision = precision; p.recall = recall; p.stats = stats;
  char* w = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t(255));
  p.pack = reinterpret_cast<unsigned char*>(w);   w += vr_align256((long)CM_CH * D);
  p.slices = reinterpret_cast<unsigned char*>(w);
  p.slice_bytes = slice_bytes;
  const hipStream_t st = vr_stream(stream);
  if (hipMemsetAsync(n_gt, 0, sizeof(int) * CM_A * num_classes, st) != hipSuccess) {
    vr_set_error("coco_map: memset failed");
    return VR_ERR_LAUNCH;
  }
  if (G > 0) {
    hipLaunchKernelGGL(cm_counts_kernel, dim3((unsigned)vr_cdiv(G, 256)), dim3(256), 0, st, p);
    VR_LAUNCH_CHECK("coco_map counts");
  }
  if (n_groups > 0) {
    hipLaunchKernelGGL(cm_match_kernel, dim3((unsigned)n_groups), dim3(64), (size_t)lds_bytes, st, p);
    VR_LAUNCH_CHECK("coco_map match");
  }
  hipLaunchKernelGGL(cm_curve_kernel, dim3(num_classes, CM_CH), dim3(CM_BLOCK), 0, st, p);
  VR_LAUNCH_CHECK("coco_map curve");
  hipLaunchKernelGGL(cm_summarise_kernel, dim3(12), dim3(CM_SUM_BLOCK), 0, st, p);
  VR_LAUNCH_CHECK("coco_map summarise");
  return VR_OK;
}
