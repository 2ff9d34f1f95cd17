// The record arena of a validation pass: what utils/callbacks.py:151-170 (`get_map_txt`) writes per image as text and
// utils_map.py parses back, appended on the device so that a captured graph can evaluate a whole validation set with one
// read-back at the end.  Two kernels, no atomics on the records (every element has one owner, so the arena holds the same
// bits on every run):
//   append   one workgroup per image b of the batch, slot = cursor + b.  The first n = min(kept[b], max_boxes) rows (already
//            in descending score order) become label = (int)class, score = the six characters `str(obj * class_conf)[:6]`
//            read back as a double, box = int() of left, top, right, bottom; the first min(gt_count[b], max_gt) ground
//            truths are copied.  With cursor + B > N the launch writes nothing.
//   advance  one thread: cursor += B, or FLAG_EVAL_CAPACITY with the cursor left alone.  It runs after `append` on the same
//            stream, so every workgroup of `append` has read the cursor it adds to.
// The six-character score without printing a float ("EvalPipeline"): x = (double)s, k = rint(x * 1e4) -- the
// product is exact, 24 x 14 bits -- and the result is k / 1e4 if that double rounds to s as a float (the shortest
// representation of s then has at most four decimals), floor(x * 1e4) / 1e4 otherwise.  Holds for 1e-4 <= s <= 1.
#include "common.h"

// s = obj * class_conf is ONE fp32 multiply and the quantisation rounds after every operation: no a*b+c fusion in this file.
#pragma clang fp contract(off)

namespace {

constexpr int EVAL_FLAG_CAPACITY = 32;       // bits of the flag word, above render.hip's 1, 2, 4 and nms.hip's 8, 16
constexpr int EVAL_FLAG_GT = 64;             // an image with more ground truths than max_gt (the first max_gt are kept)
constexpr int EVAL_FLAG_BOX = 128;           // a coordinate or class that int() cannot take: non-finite or outside int32

struct AppendArgs {
  const float* rows;           // (B, cap, 7): top, left, bottom, right, obj, class_conf, class
  const int* kept;             // (B)
  const int* gt;               // (B, max_gt, 5): x1, y1, x2, y2, class
  const int* gt_count;         // (B)
  int B, cap, max_gt, N, max_boxes;
  int* cursor;
  int* det_label;              // (N, max_boxes)
  double* det_score;           // (N, max_boxes)
  double* det_box;             // (N, max_boxes, 4): left, top, right, bottom
  int* det_count;              // (N)
  int* gt_label;               // (N, max_gt)
  double* gt_box;              // (N, max_gt, 4)
  int* gt_n;                   // (N)
  int* flag;
};

__device__ __forceinline__ bool has_room(int cursor, int B, int N) { return cursor >= 0 && (long)cursor + B <= (long)N; }

// float(str(np.float32(s))[:6]) for 1e-4 <= s <= 1
__device__ __forceinline__ double score6(float s) {
  const double x = (double)s;
  const double y = x * 1e4;
  const double q = rint(y) / 1e4;
  return (float)q == s ? q : floor(y) / 1e4;
}

// (double)int(v), Python's truncation toward zero; *bad where Python raises (NaN, inf) or the value leaves int32
__device__ __forceinline__ int trunc_i32(float v, bool* bad) {
  const double d = (double)v;
  if (!(d >= -2147483648.0 && d < 2147483648.0)) {
    *bad = true;
    return 0;
  }
  return (int)d;
}

__global__ __launch_bounds__(64) void eval_append_kernel(const AppendArgs p) {
  const int b = blockIdx.x, cursor = *p.cursor;
  if (!has_room(cursor, p.B, p.N)) return;
  const long slot = (long)cursor + b;
  const int n = min(min(max(p.kept[b], 0), p.max_boxes), p.cap);
  const int have = p.gt_count[b], g = min(max(have, 0), p.max_gt);
  bool bad = false;
  for (int k = threadIdx.x; k < n; k += 64) {
    const float* r = p.rows + ((long)b * p.cap + k) * 7;
    const long o = slot * p.max_boxes + k;
    const float s = r[4] * r[5];
    p.det_score[o] = score6(s);
    p.det_label[o] = trunc_i32(r[6], &bad);
    double* box = p.det_box + 4 * o;
    box[0] = (double)trunc_i32(r[1], &bad);
    box[1] = (double)trunc_i32(r[0], &bad);
    box[2] = (double)trunc_i32(r[3], &bad);
    box[3] = (double)trunc_i32(r[2], &bad);
  }
  for (int j = threadIdx.x; j < g; j += 64) {
    const int* t = p.gt + ((long)b * p.max_gt + j) * 5;
    const long o = slot * p.max_gt + j;
    double* box = p.gt_box + 4 * o;
    box[0] = (double)t[0]; box[1] = (double)t[1]; box[2] = (double)t[2]; box[3] = (double)t[3];
    p.gt_label[o] = t[4];
  }
  if (threadIdx.x == 0) {
    p.det_count[slot] = n;
    p.gt_n[slot] = g;
    if (have > p.max_gt) atomicOr(p.flag, EVAL_FLAG_GT);
  }
  if (bad) atomicOr(p.flag, EVAL_FLAG_BOX);
}

__global__ void eval_advance_kernel(int* cursor, int B, int N, int* flag) {
  const int c = *cursor;
  if (has_room(c, B, N)) *cursor = c + B;
  else atomicOr(flag, EVAL_FLAG_CAPACITY);
}

}  // namespace

extern "C" int vrnet_eval_append_f32(const float* rows, const int* kept, int B, int cap, const int* gt, const int* gt_count,
                                     int max_gt, int* cursor, int N, int max_boxes, int* det_label, double* det_score,
                                     double* det_box, int* det_count, int* gt_label, double* gt_box, int* gt_n, int* flag,
                                     void* stream) {
  VR_CHECK_ARG(rows && kept && gt && gt_count && cursor && det_label && det_score && det_box && det_count && gt_label &&
                   gt_box && gt_n && flag, "eval_append: every array is required");
  VR_CHECK_ARG(B > 0 && B < 65536 && cap > 0 && max_gt > 0 && N > 0 && max_boxes > 0 && (long)B * cap < (1L << 27) &&
                   (long)N * max_boxes < (1L << 31) && (long)N * max_gt < (1L << 31) && (long)B * max_gt < (1L << 27),
               "eval_append: bad shape (B %d, cap %d, max_gt %d, capacity %d, max_boxes %d)", B, cap, max_gt, N, max_boxes);
  AppendArgs p{};
  p.rows = rows; p.kept = kept; p.gt = gt; p.gt_count = gt_count;
  p.B = B; p.cap = cap; p.max_gt = max_gt; p.N = N; p.max_boxes = max_boxes;
  p.cursor = cursor; p.det_label = det_label; p.det_score = det_score; p.det_box = det_box; p.det_count = det_count;
  p.gt_label = gt_label; p.gt_box = gt_box; p.gt_n = gt_n; p.flag = flag;
  const hipStream_t st = vr_stream(stream);
  hipLaunchKernelGGL(eval_append_kernel, dim3(B), dim3(64), 0, st, p);
  VR_LAUNCH_CHECK("eval_append");
  hipLaunchKernelGGL(eval_advance_kernel, dim3(1), dim3(1), 0, st, cursor, B, N, flag);
  VR_LAUNCH_CHECK("eval_append advance");
  return VR_OK;
}
