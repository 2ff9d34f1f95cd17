// The detection metric of the evaluation callback: utils/utils_map.py:276-798 `get_map` (VOC AP matching, called at
// utils/callbacks.py:226) with `voc_ap` (:95-136) and `log_average_miss_rate` (:31-67), for T IoU thresholds at once
// (the evaluation side).  The reference marks ground truths `used` in confidence order, but the ground truth a
// detection is compared with is the arg-max IoU over ALL ground truths of its image and class, used or not (:462-477): the
// match does not depend on the order, and "the first detection to claim a ground truth is the true positive" is an integer
// atomicMin of ranks.  Five kernels, all deterministic (no result depends on the order in which workgroups or waves run):
//   groups  one thread per (image, class): the non-difficult ground truths of the group are counted into n_gt[class] and,
//           if there is one, the image into n_img[class] (integer atomics)
//   match   one thread per detection, in rank order: the reference's IoU loop over the ground truths of its image and class
//           in input order (difficult ones included), first strict maximum from ovmax = -1; per threshold that ovmax
//           reaches on a non-difficult ground truth g, atomicMin(first[t][g], rank)
//   flags   one thread per (threshold, detection): the tp / fp byte pair (:482-498)
//   curve   one workgroup per (class, threshold): a chunked block scan with a carry (wave scans through __shfl_up) gives
//           the cumulative tp / fp, from which recall / precision, the values at the score threshold and the nine
//           miss-rate look-ups follow; a reverse chunked pass (suffix maximum of the precision through __shfl_down, carry
//           from the later chunks) gives the AP terms, summed per thread in a fixed order and reduced in a fixed tree
//   mean    one thread per threshold: the mean AP over the classes that have a non-difficult ground truth, in class order
// Every decision is IEEE fp64 with one rounding per operation (pragma below) in the reference's operand order, so a
// Python-float restatement reproduces tp, fp, recall and precision bit for bit (tests/test_detmap.py).
#include "common.h"

#include <climits>
#include <cmath>

// No a*b+c fusion anywhere in this file: the IoU, recall and precision must round after every operation, as Python's floats.
#pragma clang fp contract(off)

namespace {

constexpr int DM_MAX_T = 16;
constexpr int DM_MAX_N = 1 << 24;            // detections, ground truths (ranks fit an int with room for the 0x7f fill)
constexpr int DM_MAX_CLASSES = 65535;        // grid.x of the curve kernel
constexpr long DM_MAX_GROUPS = 1L << 27;     // images x classes: the dense (image, class) -> ground-truth range table
constexpr int DM_BLOCK = 512, DM_WAVES = DM_BLOCK / 64;
constexpr int DM_KEYS = 11;                  // look-ups of the curve kernel: ctp, cfp at the score threshold + 9 fppi points

// numpy.logspace(-2.0, 0.0, num=9), to the bit (utils_map.py:60)
__constant__ double DM_FPPI_REF[9] = {0x1.47ae147ae147bp-7, 0x1.235a71c5ee5ccp-6, 0x1.030dc4ea03a72p-5,
                                      0x1.ccab8602d2696p-5, 0x1.999999999999ap-4, 0x1.6c310e3769f3fp-3,
                                      0x1.43d136248490fp-2, 0x1.1feb33c1c381ep-1, 0x1.0p+0};

struct DetMapArgs {
  const int* det_image;          // (D) input order
  const int* det_label;
  const double* det_score;
  const double* det_box;         // (D, 4) left, top, right, bottom
  const int* order;              // (D) rank -> input index: classes ascending, score descending, ties in input order
  const int* det_off;            // (C + 1) ranks of class c: det_off[c] .. det_off[c + 1] - 1
  int D;
  const double* gt_box;          // (G, 4) input order
  const unsigned char* gt_diff;  // (G)
  const int* gt_perm;            // (G) slot -> input index: grouped by image * C + class, input order inside a group
  const int* gt_off;             // (I * C + 1) slots of group k: gt_off[k] .. gt_off[k + 1] - 1
  int G, I, C, T;
  double thr[DM_MAX_T];
  double score_thr;
  int* match;                    // (D) by rank: input index of the matched ground truth, -1 = none overlaps
  double* ovmax;                 // (D) by rank
  unsigned char* tp;             // (T, D) by rank
  unsigned char* fp;
  double* rec;                   // (T, D) by rank or NULL
  double* prec;
  int* n_gt;                     // (C)
  int* n_img;                    // (C)
  int* n_tp;                     // (T, C)
  double *ap, *f1, *recall, *precision, *lamr;   // (T, C)
  double* map;                   // (T)
  int* first;                    // workspace (T, G): lowest rank matched to the ground truth at the threshold
  int* ctp;                      // workspace (T, D) by rank: inclusive cumulative tp / fp of the class
  int* cfp;
};

// Python's max(a, b) / min(a, b): the first argument unless the second is strictly greater / smaller
__device__ __forceinline__ double pymax(double a, double b) { return (b > a) ? b : a; }
__device__ __forceinline__ double pymin(double a, double b) { return (b < a) ? b : a; }

__global__ __launch_bounds__(256) void dm_groups_kernel(const DetMapArgs p) {
  const long groups = (long)p.I * p.C;
  for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < groups; k += (long)gridDim.x * 256) {
    int cnt = 0;
    for (int s = p.gt_off[k]; s < p.gt_off[k + 1]; ++s) cnt += p.gt_diff[p.gt_perm[s]] ? 0 : 1;
    if (cnt) {
      const int c = (int)(k % p.C);
      atomicAdd(p.n_gt + c, cnt);
      atomicAdd(p.n_img + c, 1);
    }
  }
}

__global__ __launch_bounds__(256) void dm_match_kernel(const DetMapArgs p) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= p.D) return;
  const int d = p.order[r];
  const int img = p.det_image[d], cls = p.det_label[d];
  const double b0 = p.det_box[4 * (long)d], b1 = p.det_box[4 * (long)d + 1], b2 = p.det_box[4 * (long)d + 2],
               b3 = p.det_box[4 * (long)d + 3];
  double ovmax = -1.0;
  int gm = -1;
  if (img >= 0 && img < p.I && cls >= 0 && cls < p.C) {          // the host checks the ranges; never index outside the table
    const long k = (long)img * p.C + cls;
    for (int s = p.gt_off[k]; s < p.gt_off[k + 1]; ++s) {
      const int g = p.gt_perm[s];
      const double g0 = p.gt_box[4 * (long)g], g1 = p.gt_box[4 * (long)g + 1], g2 = p.gt_box[4 * (long)g + 2],
                   g3 = p.gt_box[4 * (long)g + 3];
      const double iw = pymin(b2, g2) - pymax(b0, g0) + 1.0;
      const double ih = pymin(b3, g3) - pymax(b1, g1) + 1.0;
      if (iw > 0.0 && ih > 0.0) {
        const double ua = (b2 - b0 + 1.0) * (b3 - b1 + 1.0) + (g2 - g0 + 1.0) * (g3 - g1 + 1.0) - iw * ih;
        const double ov = iw * ih / ua;                            // IEEE divide: hipcc's default for fp64
        if (ov > ovmax) { ovmax = ov; gm = g; }
      }
    }
  }
  p.match[r] = gm;
  p.ovmax[r] = ovmax;
  if (gm >= 0 && !p.gt_diff[gm])
    for (int t = 0; t < p.T; ++t)
      if (ovmax >= p.thr[t]) atomicMin(p.first + (long)t * p.G + gm, r);
}

__global__ __launch_bounds__(256) void dm_flags_kernel(const DetMapArgs p) {
  const int r = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
  if (r >= p.D) return;
  const int gm = p.match[r];
  unsigned char tp = 0, fp = 0;
  if (p.ovmax[r] >= p.thr[t]) {
    if (gm < 0) fp = 1;                        // only with a threshold <= -1 (ovmax = -1 without an overlapping ground truth)
    else if (!p.gt_diff[gm]) {                 // a matched difficult ground truth: neither tp nor fp (:484)
      if (p.first[(long)t * p.G + gm] == r) tp = 1;
      else fp = 1;
    }
  } else {
    fp = 1;
  }
  p.tp[(long)t * p.D + r] = tp;
  p.fp[(long)t * p.D + r] = fp;
}

__global__ __launch_bounds__(DM_BLOCK) void dm_curve_kernel(const DetMapArgs p) {
  __shared__ int wtp[DM_WAVES], wfp[DM_WAVES];
  __shared__ double wmax[DM_WAVES], wsum[DM_WAVES];
  __shared__ unsigned long long wkey[DM_WAVES][DM_KEYS];
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lo = p.det_off[c], n = p.det_off[c + 1] - lo;
  const int ngt = p.n_gt[c], nimg = p.n_img[c];
  const long o = (long)t * p.D + lo, oc = (long)t * p.C + c;
  const double dgt = (double)max(ngt, 1), dimg = (double)nimg;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (n == 0) {
    // no detections of the class: voc_ap of empty lists is 0, every value at the score threshold and lamr are 0
    if (tid == 0) {
      const double v = ngt > 0 ? 0.0 : nan;
      p.n_tp[oc] = 0;
      p.ap[oc] = v; p.f1[oc] = v; p.recall[oc] = v; p.precision[oc] = v; p.lamr[oc] = v;
    }
    return;
  }

  // forward: inclusive cumulative tp / fp, recall / precision, the look-ups.  A look-up key is (index + 1) << 32 | count:
  // the maximum over the elements that qualify is the LAST index that qualifies together with its count, 0 = none.
  int carry_tp = 0, carry_fp = 0;
  unsigned long long key[DM_KEYS];
#pragma unroll
  for (int k = 0; k < DM_KEYS; ++k) key[k] = 0;
  for (int base = 0; base < n; base += DM_BLOCK) {
    const int i = base + tid;
    const bool v = i < n;
    int a = v ? p.tp[o + i] : 0, b = v ? p.fp[o + i] : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int ua = __shfl_up(a, off, 64), ub = __shfl_up(b, off, 64);
      if (lane >= off) { a += ua; b += ub; }
    }
    if (lane == 63) { wtp[wv] = a; wfp[wv] = b; }
    __syncthreads();
    int pa = carry_tp, pb = carry_fp;
#pragma unroll
    for (int w = 0; w < DM_WAVES; ++w) {
      const int x = wtp[w], y = wfp[w];
      if (w < wv) { pa += x; pb += y; }
      carry_tp += x; carry_fp += y;
    }
    a += pa; b += pb;
    if (v) {
      p.ctp[o + i] = a;
      p.cfp[o + i] = b;
      if (p.rec) {
        p.rec[o + i] = (double)a / dgt;
        p.prec[o + i] = (double)a / (double)max(a + b, 1);
      }
      const unsigned long long hi = (unsigned long long)(i + 1) << 32;
      // score_threhold_idx starts at 0 (:436): element 0 always qualifies, any later one that passes replaces it
      if (i == 0 || p.det_score[p.order[lo + i]] >= p.score_thr) { key[0] = hi | (unsigned)a; key[1] = hi | (unsigned)b; }
      if (nimg > 0) {
        const double fppi = (double)b / dimg;
#pragma unroll
        for (int k = 0; k < 9; ++k)
          if (fppi <= DM_FPPI_REF[k]) key[2 + k] = hi | (unsigned)a;
      }
    }
    __syncthreads();
  }

  // reverse: mpre[i] = max(prec[i ..], 0) (:118-119), AP terms where the recall changes (:125-135).  The term of the
  // appended (recall 1, precision 0) pair is a product with 0 and is left out.
  double carry = 0.0, acc = 0.0;
  for (int base = (n - 1) / DM_BLOCK * DM_BLOCK; base >= 0; base -= DM_BLOCK) {
    const int i = base + tid;
    const bool v = i < n;
    int a = 0, b = 0;
    if (v) { a = p.ctp[o + i]; b = p.cfp[o + i]; }
    double m = v ? (double)a / (double)max(a + b, 1) : 0.0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double u = __shfl_down(m, off, 64);
      if (lane + off < 64 && u > m) m = u;
    }
    if (lane == 0) wmax[wv] = m;
    __syncthreads();
    double later = carry;
#pragma unroll
    for (int w = 0; w < DM_WAVES; ++w) {
      const double x = wmax[w];
      if (w > wv && x > later) later = x;
      if (x > carry) carry = x;
    }
    if (later > m) m = later;
    if (v) {
      const int aprev = i ? p.ctp[o + i - 1] : 0;
      const double r = (double)a / dgt, rp = (double)aprev / dgt;
      if (r != rp) acc += (r - rp) * m;
    }
    __syncthreads();
  }

  // fixed-order reductions: xor tree inside a wave, then the waves in order
  acc = wave_sum(acc);
#pragma unroll
  for (int k = 0; k < DM_KEYS; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long u = __shfl_xor(key[k], off, 64);
      if (u > key[k]) key[k] = u;
    }
  }
  if (lane == 0) {
    wsum[wv] = acc;
#pragma unroll
    for (int k = 0; k < DM_KEYS; ++k) wkey[wv][k] = key[k];
  }
  __syncthreads();
  if (tid < DM_KEYS) {
    unsigned long long q = 0;
    for (int w = 0; w < DM_WAVES; ++w) q = wkey[w][tid] > q ? wkey[w][tid] : q;
    wkey[0][tid] = q;                          // row 0, column tid: read above by this thread only
  }
  __syncthreads();
  if (tid != 0) return;
  const unsigned long long* kk = wkey[0];
  double ap = 0.0;
  for (int w = 0; w < DM_WAVES; ++w) ap += wsum[w];
  p.n_tp[oc] = carry_tp;
  if (ngt <= 0) {                              // the reference evaluates only classes with a non-difficult ground truth
    p.ap[oc] = nan; p.f1[oc] = nan; p.recall[oc] = nan; p.precision[oc] = nan; p.lamr[oc] = nan;
    return;
  }
  const int a = (int)(kk[0] & 0xffffffffu), b = (int)(kk[1] & 0xffffffffu);
  const double rec = (double)a / dgt, prec = (double)a / (double)max(a + b, 1);
  const double den = prec + rec;
  p.ap[oc] = ap;
  p.recall[oc] = rec;
  p.precision[oc] = prec;
  p.f1[oc] = rec * prec * 2.0 / (den == 0.0 ? 1.0 : den);
  // lamr (:31-67): mr_tmp[j] = 1 - rec[j - 1] at the last j with fppi_tmp[j] <= ref, j = 0 being the prepended (-1, 1) pair
  double s = 0.0;
#pragma unroll 1
  for (int k = 0; k < 9; ++k) {
    const unsigned long long q = kk[2 + k];
    const double mr = q ? 1.0 - (double)(int)(q & 0xffffffffu) / dgt : 1.0;
    s += log(mr > 1e-10 ? mr : 1e-10);
  }
  p.lamr[oc] = exp(s / 9.0);
}

__global__ void dm_mean_kernel(const DetMapArgs p) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.T) return;
  double sum = 0.0;
  int cnt = 0;
  for (int c = 0; c < p.C; ++c)
    if (p.n_gt[c] > 0) { sum += p.ap[(long)t * p.C + c]; ++cnt; }
  p.map[t] = cnt ? sum / (double)cnt : 0.0;
}

}  // namespace

extern "C" long vrnet_det_map_workspace_bytes(int D, int G, int T) {
  if (D < 0 || G < 0 || T <= 0) return 0;
  return 256 + vr_align256(4L * T * G) + 2 * vr_align256(4L * T * D);
}

extern "C" int vrnet_det_map_f64(const int* det_image, const int* det_label, const double* det_score, const double* det_box,
                                 const int* order, const int* det_offsets, int D, const double* gt_box,
                                 const unsigned char* gt_difficult, const int* gt_perm, const int* gt_offsets, int G,
                                 int n_images, int num_classes, const double* min_overlap, int T, double score_threhold,
                                 int* match, double* ovmax, unsigned char* tp, unsigned char* fp, double* rec, double* prec,
                                 int* n_gt, int* n_img, int* n_tp, double* ap, double* f1, double* recall, double* precision,
                                 double* lamr, double* map, void* workspace, long workspace_bytes, void* stream) {
  VR_CHECK_ARG(D >= 0 && D <= DM_MAX_N && G >= 0 && G <= DM_MAX_N, "det_map: %d detections, %d ground truths (0..%d each)", D, G,
               DM_MAX_N);
  VR_CHECK_ARG(num_classes >= 1 && num_classes <= DM_MAX_CLASSES, "det_map: %d classes (1..%d supported)", num_classes,
               DM_MAX_CLASSES);
  VR_CHECK_ARG(n_images >= 0 && (long)n_images * num_classes <= DM_MAX_GROUPS,
               "det_map: %d images x %d classes (at most %ld (image, class) groups)", n_images, num_classes, DM_MAX_GROUPS);
  VR_CHECK_ARG(min_overlap && T >= 1 && T <= DM_MAX_T, "det_map: %d thresholds (1..%d supported)", T, DM_MAX_T);
  VR_CHECK_ARG((D == 0 && G == 0) || n_images > 0, "det_map: detections or ground truths but no image");
  VR_CHECK_ARG(det_offsets && gt_offsets && n_gt && n_img && n_tp && ap && f1 && recall && precision && lamr && map &&
                   (D == 0 || (det_image && det_label && det_score && det_box && order && match && ovmax && tp && fp)) &&
                   (G == 0 || (gt_box && gt_difficult && gt_perm)) && (!rec == !prec),
               "det_map: missing argument (rec and prec come together)");
  if (!workspace || workspace_bytes < vrnet_det_map_workspace_bytes(D, G, T)) {
    vr_set_error("det_map: workspace %ld < %ld bytes", workspace_bytes, vrnet_det_map_workspace_bytes(D, G, T));
    return VR_ERR_WORKSPACE;
  }
  DetMapArgs p{};
  p.det_image = det_image; p.det_label = det_label; p.det_score = det_score; p.det_box = det_box;
  p.order = order; p.det_off = det_offsets; p.D = D;
  p.gt_box = gt_box; p.gt_diff = gt_difficult; p.gt_perm = gt_perm; p.gt_off = gt_offsets;
  p.G = G; p.I = n_images; p.C = num_classes; p.T = T;
  for (int t = 0; t < T; ++t) p.thr[t] = min_overlap[t];
  p.score_thr = score_threhold;
  p.match = match; p.ovmax = ovmax; p.tp = tp; p.fp = fp; p.rec = rec; p.prec = prec;
  p.n_gt = n_gt; p.n_img = n_img; p.n_tp = n_tp;
  p.ap = ap; p.f1 = f1; p.recall = recall; p.precision = precision; p.lamr = lamr; p.map = map;
  char* w = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t(255));
  p.first = reinterpret_cast<int*>(w);   w += vr_align256(4L * T * G);
  p.ctp = reinterpret_cast<int*>(w);     w += vr_align256(4L * T * D);
  p.cfp = reinterpret_cast<int*>(w);
  const hipStream_t st = vr_stream(stream);
  // first = 0x7f7f7f7f: above every rank (D <= 2^24)
  if (hipMemsetAsync(n_gt, 0, sizeof(int) * num_classes, st) != hipSuccess ||
      hipMemsetAsync(n_img, 0, sizeof(int) * num_classes, st) != hipSuccess ||
      (G > 0 && hipMemsetAsync(p.first, 0x7f, sizeof(int) * (long)T * G, st) != hipSuccess)) {
    vr_set_error("det_map: memset failed");
    return VR_ERR_LAUNCH;
  }
  if (G > 0) {
    long grid = vr_cdiv((long)n_images * num_classes, 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(dm_groups_kernel, dim3((unsigned)grid), dim3(256), 0, st, p);
    VR_LAUNCH_CHECK("det_map groups");
  }
  if (D > 0) {
    hipLaunchKernelGGL(dm_match_kernel, dim3((unsigned)vr_cdiv(D, 256)), dim3(256), 0, st, p);
    VR_LAUNCH_CHECK("det_map match");
    hipLaunchKernelGGL(dm_flags_kernel, dim3((unsigned)vr_cdiv(D, 256), T), dim3(256), 0, st, p);
    VR_LAUNCH_CHECK("det_map flags");
  }
  hipLaunchKernelGGL(dm_curve_kernel, dim3(num_classes, T), dim3(DM_BLOCK), 0, st, p);
  VR_LAUNCH_CHECK("det_map curve");
  hipLaunchKernelGGL(dm_mean_kernel, dim3(1), dim3(64), 0, st, p);
  VR_LAUNCH_CHECK("det_map mean");
  return VR_OK;
}
