// Input formats of the training pipeline on the device: what YoloDataset.__getitem__ and
// yolo_dataset_collate (utils/dataloader.py:88-107, 440-457) do to a batch AFTER the host-side letterbox -- normalise the
// RGB image (utils_seg/utils.py:43-47 preprocess_input: /255, - mean, / std, in float64), HWC -> CHW, cast to float32;
// clamp the label map to the ignore class (:96-97) and expand it to one-hot with the extra channel (:103-105).  The host
// hands over the letterboxed batch as BYTES (image 3 B / pixel, label 1 B / pixel) instead of the float64 -> float32 tensors
// the reference's loader ships: (12 + 8 + 4 (nc + 1)) B per pixel become 4 B over PCIe (8.4 MB instead of 126 MB for a
// batch of 8 at 512 x 512 with 9 classes), and the one-hot expansion -- np.eye indexing on the host in the reference --
// is a store pattern here.  One thread per pixel; every output store is coalesced (CHW planes, label, one-hot rows).
// The image arithmetic is done in double and rounded once, as numpy does it: results are bit-identical to the reference's.
// vrnet_radar_normalise is the radar half of the prediction scripts: utils/utils.py:50-53 preprocess_input_radar, the
// min-max normalisation yolo.py:134 applies to each frame's (4, H, W) maps on the host, as two launches -- per-frame
// (min, max) partials, then the apply, each workgroup folding the frame's partials first.  Min and max are exact, so the
// order of the reduction does not matter; a NaN anywhere in a frame makes both NaN, as np.min / np.max do.  The arithmetic
// runs in the maps' own type, as numpy's does (a float32 array stays float32 against the Python scalar 1e-13).
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void batch_formats_kernel(const unsigned char* img, const unsigned char* png, long npix,
                                                            long HW, int ns, float* images, long long* png_out,
                                                            float* onehot) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= npix) return;
  if (img) {
    const double mean[3] = {0.485, 0.456, 0.406}, sd[3] = {0.229, 0.224, 0.225};
    const long b = e / HW, p = e - b * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double v = (double)img[e * 3 + c];
      v /= 255.0;
      v -= mean[c];
      v /= sd[c];
      images[(b * 3 + c) * HW + p] = (float)v;
    }
  }
  if (png) {
    int lab = png[e];
    if (lab >= ns) lab = ns;
    if (png_out) png_out[e] = lab;
    if (onehot) {
      float* row = onehot + e * (ns + 1);
      for (int c = 0; c <= ns; ++c) row[c] = c == lab ? 1.f : 0.f;
    }
  }
}

constexpr int RD_PARTS = 64;          // (min, max) partials per frame: one wave folds them

template <typename T>
struct MinMax {
  T lo, hi;
};

// NaN-propagating fold of two (min, max) pairs
template <typename T>
__device__ __forceinline__ MinMax<T> mm_fold(const MinMax<T> a, const MinMax<T> b) {
  MinMax<T> r;
  r.lo = (a.lo != a.lo) ? a.lo : ((b.lo != b.lo || b.lo < a.lo) ? b.lo : a.lo);
  r.hi = (a.hi != a.hi) ? a.hi : ((b.hi != b.hi || b.hi > a.hi) ? b.hi : a.hi);
  return r;
}

template <typename T>
__device__ __forceinline__ MinMax<T> mm_wave(MinMax<T> v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    MinMax<T> w;
    w.lo = __shfl_xor(v.lo, o, 64);
    w.hi = __shfl_xor(v.hi, o, 64);
    v = mm_fold(v, w);
  }
  return v;
}

template <typename T>
__global__ __launch_bounds__(256) void radar_minmax_kernel(const T* x, long n, int parts, T* part) {
  __shared__ T s_lo[4], s_hi[4];
  const T* f = x + (long)blockIdx.y * n;
  MinMax<T> v{(T)INFINITY, (T)-INFINITY};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)parts * 256) v = mm_fold(v, MinMax<T>{f[i], f[i]});
  v = mm_wave(v);
  if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = v.lo; s_hi[threadIdx.x >> 6] = v.hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) v = mm_fold(v, MinMax<T>{s_lo[w], s_hi[w]});
    T* o = part + ((long)blockIdx.y * parts + blockIdx.x) * 2;
    o[0] = v.lo;
    o[1] = v.hi;
  }
}

// out = float32((x - lo) / (hi - lo) + 1e-13) in T, one rounding per operation; part NULL: the plain cast
template <typename T>
__global__ __launch_bounds__(256) void radar_apply_kernel(const T* x, long n, int parts, const T* part, float* out) {
  __shared__ T s_mm[2];
  const long off = (long)blockIdx.y * n;
  T lo = 0, range = 1;
  if (part) {
    if (threadIdx.x < 64) {
      MinMax<T> v{(T)INFINITY, (T)-INFINITY};
      if ((int)threadIdx.x < parts) {
        const T* q = part + ((long)blockIdx.y * parts + threadIdx.x) * 2;
        v = MinMax<T>{q[0], q[1]};
      }
      v = mm_wave(v);
      if (threadIdx.x == 0) { s_mm[0] = v.lo; s_mm[1] = v.hi; }
    }
    __syncthreads();
    lo = s_mm[0];
    range = s_mm[1] - lo;
  }
  const T eps = (T)0.0000000000001;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const T v = x[off + i];
    out[off + i] = part ? (float)((v - lo) / range + eps) : (float)v;
  }
}

template <typename T>
int radar_launch(const T* x, int B, long n, int normalise, T* part, float* out, hipStream_t st) {
  const int parts = (int)(vr_cdiv(n, 256) < RD_PARTS ? vr_cdiv(n, 256) : RD_PARTS);
  if (normalise) {
    hipLaunchKernelGGL(radar_minmax_kernel<T>, dim3(parts, B), dim3(256), 0, st, x, n, parts, part);
    VR_LAUNCH_CHECK("radar_normalise (min, max)");
  }
  const long grid = vr_cdiv(n, 256) < 1024 ? vr_cdiv(n, 256) : 1024;
  hipLaunchKernelGGL(radar_apply_kernel<T>, dim3((unsigned)grid, B), dim3(256), 0, st, x, n, parts,
                     normalise ? (const T*)part : (const T*)nullptr, out);
  VR_LAUNCH_CHECK("radar_normalise");
  return VR_OK;
}

}  // namespace

extern "C" long vrnet_radar_workspace_bytes(int B) { return B > 0 ? (long)B * RD_PARTS * 2 * sizeof(double) : 0; }

extern "C" int vrnet_radar_normalise(const void* radar, int is_f64, int B, long frame_elems, int normalise, float* out,
                                     void* workspace, long workspace_bytes, void* stream) {
  VR_CHECK_ARG(radar && out && B > 0 && B < 65536 && frame_elems > 0 && (const void*)out != radar,
               "radar_normalise: bad arguments (B %d, %ld values per frame)", B, frame_elems);
  VR_CHECK_ARG(!normalise || ((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && workspace &&
                              workspace_bytes >= vrnet_radar_workspace_bytes(B)),
               "radar_normalise: workspace %ld < %ld", workspace_bytes, vrnet_radar_workspace_bytes(B));
  const hipStream_t st = vr_stream(stream);
  return is_f64 ? radar_launch(static_cast<const double*>(radar), B, frame_elems, normalise, static_cast<double*>(workspace), out, st)
                : radar_launch(static_cast<const float*>(radar), B, frame_elems, normalise, static_cast<float*>(workspace), out, st);
}

extern "C" int vrnet_batch_formats_u8(const unsigned char* img, const unsigned char* png, int B, int H, int W,
                                      int num_classes_seg, float* images, long long* png_out, float* onehot, void* stream) {
  VR_CHECK_ARG(B > 0 && H > 0 && W > 0, "batch_formats: bad shape");
  VR_CHECK_ARG(img || png, "batch_formats: nothing to convert");
  VR_CHECK_ARG(!img || images, "batch_formats: image bytes without an output");
  VR_CHECK_ARG(!png || ((png_out || onehot) && num_classes_seg > 0 && num_classes_seg < 255),
               "batch_formats: label bytes need an output and 0 < num_classes_seg < 255");
  const long npix = (long)B * H * W;
  hipLaunchKernelGGL(batch_formats_kernel, dim3((unsigned)vr_cdiv(npix, 256)), dim3(256), 0, vr_stream(stream), img, png,
                     npix, (long)H * W, num_classes_seg, images, png_out, onehot);
  VR_LAUNCH_CHECK("batch_formats");
  return VR_OK;
}
