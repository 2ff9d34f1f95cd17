// Segmentation post-processing of the seg logits: the class map of utils_seg/callbacks.py:113-160 `get_miou_png` /
// deeplab.py:141-167 `detect_image`, and the confusion matrix of utils_seg/utils_metrics.py:35-44 `fast_hist`.
//   softmax   one thread per pixel of the letterbox window: softmax over the C channels of the NCHW logits, written to
//             the workspace as planes (B, C, nh, nw) fp32, computed once per window pixel rather than once per tap
//   resize    one thread per output pixel: OpenCV INTER_LINEAR coordinates per axis, the 4 taps blended horizontally then
//             vertically, class by class, arg-max with the lower class first on equal values (numpy argmax); one byte out.
//             Planes, not pixel-major rows: neighbouring output pixels share or neighbour their taps, so one class's tap
//             loads of a wave fall in one or two cache lines (pixel-major rows of C floats spread them over C times as many)
//   hist      (label, pred) pair counts in a per-workgroup LDS histogram (n <= 32: 4 KiB), then one 64-bit atomic per
//             non-empty bin; integer atomics only, so the result does not depend on the order in which workgroups run
// The f_score metric (utils_metrics.py:12-31) sits next to the seg loss in loss.hip.
#include "common.h"
#include "pixel.h"                   // linear_tap: the OpenCV INTER_LINEAR tap of one axis, shared with heatmap.hip

// The source coordinate is computed in fp32 with one rounding per operation, as the rule it implements states; a fused
// multiply-add could move floor() across an integer and pick another tap.
#pragma clang fp contract(off)

namespace {

constexpr int SEGP_MAXC = 32;        // the seg loss's class cap (SMAXC in loss.hip)
constexpr int HIST_MAXN = 32;

// One body for both entry points.  The window and the size of image b are `geom` (vrnet_seg_predict_f32: one record for
// every image, ih, iw = ihm, iwm) or tab[b] clamped by vr_geom_load (vrnet_seg_predict_ragged_f32: RAGGED); the class map
// is (B, ihm, iwm) with image b in the top-left corner of its slot and 0 outside it.  The image is blockIdx.x / bpi, so a
// block reads one record and its loads are wave-uniform.
struct SegPredArgs {
  const float* x;                    // (B, C, H, W)
  const vrnet_frame_geom* tab;       // RAGGED: (B) records
  vrnet_frame_geom geom;             // otherwise: the record of every image
  int B, C, H, W, ihm, iwm;
  long pslot;                        // floats from one image's planes to the next: C * nh * nw (tight), or C * H * W
  int bpi;                           // blocks per image of this launch
  float* prob;                       // image b: (C, seg_nh, seg_nw) at b * pslot
  unsigned char* out;                // (B, ihm, iwm)
  int* flag;                         // or null
};

template <bool RAGGED>
__device__ __forceinline__ vrnet_frame_geom segp_geom(const SegPredArgs& p, int b, bool& bad) {
  bad = false;
  if constexpr (RAGGED) return vr_geom_load(p.tab, b, p.ihm, p.iwm, p.H, p.W, bad);
  return p.geom;
}

// softmax over the C channels of one pixel: src / dst step by a plane per channel
__device__ __forceinline__ void softmax_pixel(const float* src, long plane, int C, float* dst, long dplane) {
  float m = -INFINITY;
  for (int c = 0; c < C; ++c) m = fmaxf(m, src[c * plane]);
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(src[c * plane] - m);
  for (int c = 0; c < C; ++c) dst[c * dplane] = expf(src[c * plane] - m) / s;
}

template <bool RAGGED>
__global__ __launch_bounds__(256) void segp_softmax_kernel(const SegPredArgs p) {
  const long b = blockIdx.x / p.bpi, r = (long)(blockIdx.x - b * p.bpi) * 256 + threadIdx.x;
  bool bad;
  const vrnet_frame_geom g = segp_geom<RAGGED>(p, (int)b, bad);
  if (r == 0 && bad && p.flag) atomicOr(p.flag, VR_FLAG_GEOMETRY);
  const long n = (long)g.seg_nh * g.seg_nw;
  if (r >= n) return;
  const int y = (int)(r / g.seg_nw), xx = (int)(r - (long)y * g.seg_nw);
  const long plane = (long)p.H * p.W;
  softmax_pixel(p.x + b * p.C * plane + (long)(g.seg_top + y) * p.W + (g.seg_left + xx), plane, p.C,
                p.prob + b * p.pslot + r, n);
}

// output pixel (oy, ox) of one image: the arg-max over the classes of the bilinear blend of prob (C, nh, nw)
__device__ __forceinline__ unsigned char resize_argmax_pixel(const float* prob, int C, int nh, int nw, float sy, float sx,
                                                             int oy, int ox) {
  int y0, y1, x0, x1;
  float fy, fx;
  linear_tap(oy, sy, nh, y0, y1, fy);
  linear_tap(ox, sx, nw, x0, x1, fx);
  const float ax0 = 1.f - fx, ay0 = 1.f - fy;
  const long pl = (long)nh * nw;
  const float* r0 = prob + (long)y0 * nw;
  const float* r1 = prob + (long)y1 * nw;
  float best = 0.f;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    const float top = r0[c * pl + x0] * ax0 + r0[c * pl + x1] * fx;
    const float bot = r1[c * pl + x0] * ax0 + r1[c * pl + x1] * fx;
    const float v = top * ay0 + bot * fy;
    if (c == 0 || v > best) { best = v; arg = c; }
  }
  return (unsigned char)arg;
}

template <bool RAGGED>
__global__ __launch_bounds__(256) void segp_resize_argmax_kernel(const SegPredArgs p) {
  const long b = blockIdx.x / p.bpi, e = (long)(blockIdx.x - b * p.bpi) * 256 + threadIdx.x;
  bool bad;
  const vrnet_frame_geom g = segp_geom<RAGGED>(p, (int)b, bad);
  const long slot = (long)p.ihm * p.iwm;
  if (e >= slot) return;
  const int oy = (int)(e / p.iwm), ox = (int)(e - (long)oy * p.iwm);
  unsigned char cls = 0;                           // the padding of the slot, and an image without a window
  if (oy < g.ih && ox < g.iw && g.seg_nh > 0 && g.seg_nw > 0)
    cls = resize_argmax_pixel(p.prob + b * p.pslot, p.C, g.seg_nh, g.seg_nw, (float)g.seg_nh / (float)g.ih,
                              (float)g.seg_nw / (float)g.iw, oy, ox);
  p.out[b * slot + e] = cls;
}

// the two launches of both entry points; `win`: the largest window of an image, in pixels
template <bool RAGGED>
void segp_launch(SegPredArgs p, long win, hipStream_t st) {
  p.bpi = (int)vr_cdiv(win, 256);
  hipLaunchKernelGGL(segp_softmax_kernel<RAGGED>, dim3((unsigned)((long)p.B * p.bpi)), dim3(256), 0, st, p);
  p.bpi = (int)vr_cdiv((long)p.ihm * p.iwm, 256);
  hipLaunchKernelGGL(segp_resize_argmax_kernel<RAGGED>, dim3((unsigned)((long)p.B * p.bpi)), dim3(256), 0, st, p);
}

template <typename TL, typename TP>
__global__ __launch_bounds__(256) void confusion_hist_kernel(const TL* label, const TP* pred, long N, int n,
                                                             unsigned long long* hist) {
  __shared__ unsigned int bins[HIST_MAXN * HIST_MAXN];
  for (int i = threadIdx.x; i < n * n; i += 256) bins[i] = 0u;
  __syncthreads();
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < N; e += (long)gridDim.x * 256) {
    const long long a = (long long)label[e], b = (long long)pred[e];
    if (a >= 0 && a < n && b >= 0 && b < n) atomicAdd(&bins[a * n + b], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n * n; i += 256)
    if (bins[i]) atomicAdd(&hist[i], (unsigned long long)bins[i]);
}

template <typename TL>
void launch_hist(const TL* label, const void* pred, int pred_bytes, long N, int n, long long* hist, int grid,
                 hipStream_t st) {
  auto* h = reinterpret_cast<unsigned long long*>(hist);
  if (pred_bytes == 1)
    hipLaunchKernelGGL((confusion_hist_kernel<TL, unsigned char>), dim3(grid), dim3(256), 0, st, label,
                       static_cast<const unsigned char*>(pred), N, n, h);
  else
    hipLaunchKernelGGL((confusion_hist_kernel<TL, long long>), dim3(grid), dim3(256), 0, st, label,
                       static_cast<const long long*>(pred), N, n, h);
}

}  // namespace

extern "C" long vrnet_seg_predict_workspace(int B, int C, int nh, int nw) {
  return (long)B * nh * nw * C * (long)sizeof(float) + 256;
}

extern "C" int vrnet_seg_predict_f32(const float* x, int B, int C, int H, int W, int top, int left, int nh, int nw, int oh,
                                     int ow, unsigned char* out, void* workspace, long workspace_bytes, void* stream) {
  VR_CHECK_ARG(x && out && workspace && B > 0 && C > 0 && C <= SEGP_MAXC && H > 0 && W > 0 && nh > 0 && nw > 0 && top >= 0 &&
                   left >= 0 && (long)top + nh <= H && (long)left + nw <= W && oh > 0 && ow > 0,
               "seg_predict: bad arguments (1..%d classes; the window top %d left %d %d x %d must lie inside %d x %d; "
               "output %d x %d)", SEGP_MAXC, top, left, nh, nw, H, W, oh, ow);
  if (workspace_bytes < vrnet_seg_predict_workspace(B, C, nh, nw)) {
    vr_set_error("seg_predict: workspace %ld < %ld bytes", workspace_bytes, vrnet_seg_predict_workspace(B, C, nh, nw));
    return VR_ERR_WORKSPACE;
  }
  SegPredArgs p{};
  p.x = x; p.B = B; p.C = C; p.H = H; p.W = W; p.ihm = oh; p.iwm = ow;
  p.geom.ih = oh; p.geom.iw = ow; p.geom.seg_top = top; p.geom.seg_left = left; p.geom.seg_nh = nh; p.geom.seg_nw = nw;
  p.pslot = (long)C * nh * nw;
  p.prob = reinterpret_cast<float*>(workspace);
  p.out = out;
  segp_launch<false>(p, (long)nh * nw, vr_stream(stream));
  VR_LAUNCH_CHECK("seg_predict");
  return VR_OK;
}

extern "C" int vrnet_confusion_hist(const void* label, int label_bytes, const void* pred, int pred_bytes, long N, int n,
                                    long long* hist, void* stream) {
  VR_CHECK_ARG(hist && N >= 0 && n > 0 && n <= HIST_MAXN && (label_bytes == 1 || label_bytes == 8) &&
                   (pred_bytes == 1 || pred_bytes == 8) && (N == 0 || (label && pred)),
               "confusion_hist: bad arguments (1..%d classes; labels and predictions of 1 or 8 bytes)", HIST_MAXN);
  if (N == 0) return VR_OK;
  long grid = vr_cdiv(N, 256 * 8);
  if (grid > 1024) grid = 1024;
  hipStream_t st = vr_stream(stream);
  if (label_bytes == 1)
    launch_hist(static_cast<const unsigned char*>(label), pred, pred_bytes, N, n, hist, (int)grid, st);
  else
    launch_hist(static_cast<const long long*>(label), pred, pred_bytes, N, n, hist, (int)grid, st);
  VR_LAUNCH_CHECK("confusion_hist");
  return VR_OK;
}

extern "C" long vrnet_seg_predict_ragged_workspace(int B, int C, int H, int W) {
  return (long)B * H * W * C * (long)sizeof(float) + 256;
}

extern "C" int vrnet_seg_predict_ragged_f32(const float* x, const vrnet_frame_geom* geom, int B, int C, int H, int W, int ihm,
                                            int iwm, unsigned char* out, int* flag, void* workspace, long workspace_bytes,
                                            void* stream) {
  VR_CHECK_ARG(x && geom && out && workspace && B > 0 && B < 65536 && C > 0 && C <= SEGP_MAXC && H > 0 && W > 0 && ihm > 0 &&
                   iwm > 0 && (long)H * W < (1L << 31) && (long)ihm * iwm < (1L << 31),
               "seg_predict_ragged: bad arguments (B %d, 1..%d classes, got %d; logits %d x %d; slots %d x %d)", B, SEGP_MAXC, C,
               H, W, ihm, iwm);
  if (workspace_bytes < vrnet_seg_predict_ragged_workspace(B, C, H, W)) {
    vr_set_error("seg_predict_ragged: workspace %ld < %ld bytes", workspace_bytes, vrnet_seg_predict_ragged_workspace(B, C, H, W));
    return VR_ERR_WORKSPACE;
  }
  SegPredArgs p{};
  p.x = x; p.tab = geom; p.B = B; p.C = C; p.H = H; p.W = W; p.ihm = ihm; p.iwm = iwm;
  p.pslot = (long)C * H * W;
  p.prob = reinterpret_cast<float*>(workspace);
  p.out = out; p.flag = flag;
  segp_launch<true>(p, (long)H * W, vr_stream(stream));
  VR_LAUNCH_CHECK("seg_predict_ragged");
  return VR_OK;
}
