// Shared helpers for libvrnet_hip.so (gfx950 / CDNA4 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#define VR_OK 0
#define VR_ERR_ARG 1
#define VR_ERR_LAUNCH 2
#define VR_ERR_WORKSPACE 3

void vr_set_error(const char* fmt, ...);
void vr_note_kernel(int id);
// Tuning knobs and timing ablations exist ONLY in the diagnostic build (make tuning -> libvrnet_hip_tuning.so, compiled
// with -DVR_TUNING and loaded through VRNET_HIP_LIB): the product library reads no environment variable at all.
//   vr_tune("VRNET_X", d): integer knob, d in the product build.
//   vr_ablated(group): VRNET_ABLATE = comma list of kernel groups whose launches are skipped (results are garbage,
//   timing valid) -- igemm, wgrad, moments, affine, cluster, coef, spatial; always false in the product build.
#ifdef VR_TUNING
int vr_tune(const char* name, int dflt);
bool vr_ablated(const char* group);
#else
static inline int vr_tune(const char*, int dflt) { return dflt; }
static inline bool vr_ablated(const char*) { return false; }
#endif

#define VR_CHECK_ARG(cond, ...)                 \
  do {                                          \
    if (!(cond)) {                              \
      vr_set_error(__VA_ARGS__);                \
      return VR_ERR_ARG;                        \
    }                                           \
  } while (0)

#define VR_LAUNCH_CHECK(name)                                                   \
  do {                                                                          \
    hipError_t e_ = hipGetLastError();                                          \
    if (e_ != hipSuccess) {                                                     \
      vr_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));       \
      return VR_ERR_LAUNCH;                                                     \
    }                                                                           \
  } while (0)

static inline hipStream_t vr_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline long vr_cdiv(long a, long b) { return (a + b - 1) / b; }
// Workgroups of the XCD-aware tile map for mt x nt tiles: the row tiles are padded to whole eights (one per XCD).
static inline long vr_xcd_tiles(long mt, long nt) { return 8 * vr_cdiv(mt, 8) * nt; }
// workspace parts begin on 256-byte boundaries
static inline long vr_align256(long n) { return (n + 255) & ~255L; }
static inline bool vr_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// stream_ops.hip: the work split of the moments kernel on 16-byte accesses (C % 4 == 0), and the launch that finishes its
// chunk partials [B][nchunks][C][2] into out [B][C][2]
void vr_moments_plan4(int B, long HW, int C, int* TPR, int* ncb, int* nchunks, long* rows);
int vr_moments_reduce(const double* partial, double* out, int B, int nchunks, int C, hipStream_t st);
extern "C" long vrnet_moments_workspace(int B, long HW, int C);

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

extern "C" {
/* include/vrnet_hip.h: optional bf16-plane output of a producing kernel (csrc/pgemm.hip: plane tensors). */
typedef struct vrnet_planes_out {
  void* p;          /* plane q of element (row, c) at p[q * plane + row * ld + c], bf16 */
  long ld, plane;   /* row and plane stride in elements (multiples of 4; 8 to feed the plane GEMMs) */
  int np;           /* 3: the fp32 value split exactly into three planes; 1: rounded to bf16 */
} vrnet_planes_out;
}
extern "C" {
/* include/vrnet_hip.h: the per-image geometry record of the ragged (mixed-size) entry points. */
typedef struct vrnet_frame_geom {
  int ih, iw;                                   /* the image's own size inside its (ihm, iwm) slot */
  int nw, nh, dx, dy;                           /* data.letterbox_geometry: the letterbox window in the (H, W) canvas */
  int seg_top, seg_left, seg_nh, seg_nw;        /* decode.seg_window */
  int thickness;                                /* yolo.py:164 */
  int reserved;                                 /* 0 */
  double offset_y, offset_x, scale_y, scale_x;  /* infer.unmap_scalars */
} vrnet_frame_geom;
}
#define VR_FLAG_GEOMETRY 256                    /* a record that had to be clamped; bits 1..128: render / nms / evalacc */
#define VR_FLAG_BOX_COUNT 512                   /* traintargets.hip: a box count outside [0, max_gt], clamped */
#define VR_FLAG_POINT_COUNT 1024                /* radarmap.hip: a point count outside [0, max_points], clamped */
/* 2048: LB_FLAG_SCORE of labels.hip, which shares the pipeline's flag word */
#define VR_FLAG_CROP_ARENA 4096                 /* crops.hip: a crop that did not fit into the arena, dropped */
#define VR_FLAG_DEHAZE 8192                     /* dehaze.hip: a degenerate image, returned unchanged */
#define VR_FLAG_ACE 16384                       /* ace.hip: a degenerate image, returned unchanged */
#define VR_FLAG_TRACK_FULL 32768                /* track.hip: a valid row found no free slot in the track table, id 0 */
#define VR_FLAG_CAPTION 65536                   /* captions.hip: a range or a speed that cannot be drawn, left out of its caption */
#define VR_FLAG_REGIONS 131072                  /* regions.hip: more regions than the table holds; labels and head are complete */
#define VR_FLAG_JPEG_ARENA 262144               /* jpeg.hip: a file that did not fit its slot of the arena, length 0 */
extern "C" {
/* include/vrnet_hip.h: one record per region of vrnet_seg_regions_u8. */
typedef struct vrnet_region {
  int cls, area;                                /* the class of the region's pixels and their number */
  int left, top, right, bottom;                 /* the bounding box, right and bottom exclusive */
  int first;                                    /* y iw + x of the first pixel in raster order */
  int det;                                      /* the linked row of the image, -1: none */
  long long sum_x, sum_y;                       /* exact sums of the pixel coordinates: the centroid is sum / area */
} vrnet_region;
}
static_assert(sizeof(vrnet_region) == 48 && offsetof(vrnet_region, first) == 24 && offsetof(vrnet_region, det) == 28 &&
                  offsetof(vrnet_region, sum_x) == 32 && offsetof(vrnet_region, sum_y) == 40,
              "vrnet_region is 48 bytes: decode.REGION_DTYPE mirrors it");
extern "C" {
/* include/vrnet_hip.h: one record per draw row of vrnet_crop_boxes_u8. */
typedef struct vrnet_crop_rec {
  int offset;                                   /* the crop's first pixel in the arena; 0 if empty, -1 if dropped */
  int w, h;                                     /* 0, 0: an empty crop */
  int image;                                    /* the image the row belongs to; -1 behind the last row */
} vrnet_crop_rec;
}
static_assert(sizeof(vrnet_crop_rec) == 16 && offsetof(vrnet_crop_rec, offset) == 0 && offsetof(vrnet_crop_rec, w) == 4 &&
                  offsetof(vrnet_crop_rec, h) == 8 && offsetof(vrnet_crop_rec, image) == 12,
              "vrnet_crop_rec is four int32: render.CROP_RECORD mirrors it");
extern "C" {
/* include/vrnet_hip.h: one record per draw row of vrnet_chip_boxes_u8. */
typedef struct vrnet_chip_rec {
  int image;                                    /* the image the row belongs to; -1 behind the last row */
  int w, h;                                     /* the clamped crop; 0, 0: an empty crop */
  int nw, nh, dx, dy;                           /* the resized crop and where it is pasted in the chip */
  int state;                                    /* 1 resized, 2 empty (a grey chip), 0 behind the last row (not written) */
} vrnet_chip_rec;
}
static_assert(sizeof(vrnet_chip_rec) == 32 && offsetof(vrnet_chip_rec, image) == 0 && offsetof(vrnet_chip_rec, nw) == 12 &&
                  offsetof(vrnet_chip_rec, state) == 28,
              "vrnet_chip_rec is eight int32: render.CHIP_RECORD mirrors it");

__device__ __forceinline__ int vr_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Record b of the table, clamped so that no access derived from it leaves the image's slot (ihm x iwm) or the canvas
// (H x W; H == 0: the entry point has no canvas and its window fields stay as they are).  bad: something was clamped.
// b is the block's image index, so the loads are wave-uniform.
__device__ __forceinline__ vrnet_frame_geom vr_geom_load(const vrnet_frame_geom* tab, int b, int ihm, int iwm, int H, int W,
                                                          bool& bad) {
  const vrnet_frame_geom t = tab[b];
  vrnet_frame_geom g = t;
  g.ih = vr_clampi(t.ih, 0, ihm);
  g.iw = vr_clampi(t.iw, 0, iwm);
  g.thickness = vr_clampi(t.thickness, 1, 1 << 24);
  // an image without pixels is no legal record either: it stays empty (its slot is all padding) and is reported
  bad = g.ih != t.ih || g.iw != t.iw || g.thickness != t.thickness || t.ih <= 0 || t.iw <= 0;
  if (H > 0) {
    g.nw = vr_clampi(t.nw, 0, W);
    g.nh = vr_clampi(t.nh, 0, H);
    g.dx = vr_clampi(t.dx, 0, W - g.nw);
    g.dy = vr_clampi(t.dy, 0, H - g.nh);
    g.seg_nw = vr_clampi(t.seg_nw, 0, W);
    g.seg_nh = vr_clampi(t.seg_nh, 0, H);
    g.seg_left = vr_clampi(t.seg_left, 0, W - g.seg_nw);
    g.seg_top = vr_clampi(t.seg_top, 0, H - g.seg_nh);
    bad = bad || g.nw != t.nw || g.nh != t.nh || g.dx != t.dx || g.dy != t.dy || g.seg_nw != t.seg_nw || g.seg_nh != t.seg_nh ||
          g.seg_left != t.seg_left || g.seg_top != t.seg_top;
  }
  return g;
}

// The size rule of vr_geom_load alone, for the stages that read nothing else of a record: (gh, gw) clamped to the slot.
// bad: something was clamped, or a side is not positive.
__device__ __forceinline__ void vr_size_clamp(int gh, int gw, int ihm, int iwm, int& ih, int& iw, bool& bad) {
  ih = vr_clampi(gh, 0, ihm);
  iw = vr_clampi(gw, 0, iwm);
  bad = gh <= 0 || gw <= 0 || ih != gh || iw != gw;
}
// The size of image b inside its (ihm, iwm) slot: the table's under that rule; (ih0, iw0) without a table.
__device__ __forceinline__ void vr_image_size(const vrnet_frame_geom* geom, int b, int ihm, int iwm, int ih0, int iw0, int& ih,
                                              int& iw, bool& bad) {
  ih = ih0; iw = iw0; bad = false;
  if (geom) vr_size_clamp(geom[b].ih, geom[b].iw, ihm, iwm, ih, iw, bad);
}

// The draw rows of image b in a table of n_rows: offsets[b] .. offsets[b + 1], clamped so that no row lies outside it.
__device__ __forceinline__ void vr_row_range(const int* offsets, int b, int n_rows, int& start, int& n) {
  start = vr_clampi(offsets[b], 0, n_rows);
  n = vr_clampi(offsets[b + 1], start, n_rows) - start;
}

// Pillow's nearest resize of an axis in -> out (Geometry.c ImagingScaleAffine): the source index of each output index, a
// running double sum (not x * a0), so it is sequential: one thread runs it.  Shared by the label half of the letterbox
// (csrc/letterbox.hip) and the segmentation targets of the training step (csrc/traintargets.hip).
__device__ inline void vr_nearest_indices(int in, int out, int* idx) {
  const double a0 = (double)in / out;
  double xo = a0 * 0.5;
  for (int x = 0; x < out; ++x) {
    idx[x] = (int)xo;
    xo += a0;
  }
}

static inline bool vr_planes_out_ok(const vrnet_planes_out* o, int C) {
  return !o || (o->p && (o->np == 1 || o->np == 3) && o->ld >= C && o->ld % 4 == 0 && (o->np == 1 || o->plane % 4 == 0) &&
                (reinterpret_cast<uintptr_t>(o->p) & 7) == 0);
}

// Four consecutive fp32 values -> bf16 planes (8 bytes per plane): np = 3 splits each value exactly, v = p0 + p1 + p2 with
// round-to-nearest-even at each step (the residuals v - p0 and v - p0 - p1 are exact in fp32 and the last one has at most 8
// significant bits); np = 1 rounds to bf16.  All arithmetic per component (no packed fp32 with operand broadcast).
typedef __bf16 vr_bf16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void vr_store_planes4(unsigned short* dst, long plane, int np, const f32x4 v) {
  const vr_bf16x4 p0 = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
  *reinterpret_cast<vr_bf16x4*>(dst) = p0;
  if (np == 3) {
    const float r0 = v[0] - (float)p0[0], r1 = v[1] - (float)p0[1], r2 = v[2] - (float)p0[2], r3 = v[3] - (float)p0[3];
    const vr_bf16x4 p1 = {(__bf16)r0, (__bf16)r1, (__bf16)r2, (__bf16)r3};
    *reinterpret_cast<vr_bf16x4*>(dst + plane) = p1;
    const vr_bf16x4 p2 = {(__bf16)(r0 - (float)p1[0]), (__bf16)(r1 - (float)p1[1]), (__bf16)(r2 - (float)p1[2]),
                          (__bf16)(r3 - (float)p1[3])};
    *reinterpret_cast<vr_bf16x4*>(dst + 2 * plane) = p2;
  }
}


__device__ __forceinline__ float vr_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }
// exact-erf GELU (nn.GELU default, vr_coc.py:204) and its derivative.  erf is evaluated branch-free as
//   erf(z) = 1 - Q(s) exp(-z^2),  s = p z / (1 + p z),  Q a degree-6 polynomial with Q(0) = 1      (z = |u| / sqrt 2)
// (the Abramowitz-Stegun 7.1.26 form, re-fitted: 1.5e-9 maximum error in exact arithmetic, tools/fit_erf.py).  In fp32 the
// resulting GELU / GELU' deviate from the exact functions by at most 3.0e-7 / 1.4e-7 absolute -- the same as torch's own
// 0.5 x (1 + erff(x / sqrt 2)) in fp32 (4.5e-7 / 1.4e-7) -- at 18 VALU operations instead of the ~55 of the library erff with
// its two divergent branches (the GELU epilogues were VALU-bound on it).  Written in s rather than t = 1 / (1 + p z): near
// z = 0 a rounding error in t is amplified by Q'(0) ~ 3.4, an error in s is proportional to z.  exp(-z^2) = exp(-u^2 / 2) is
// also the Gaussian of the derivative.
__device__ __forceinline__ float vr_erf_abs(float u, float& gauss) {      // erf(|u| / sqrt 2); gauss = exp(-u^2 / 2)
  // (clamped: u = +-Inf must give s = 1, not Inf * 0; a NaN still propagates through the Gaussian)
  const float pz = fminf(fabsf(u) * (0.37458086389741496f * 0.70710678118654752f), 1e30f);
  const float s = pz * __builtin_amdgcn_rcpf(pz + 1.0f);
  gauss = __builtin_amdgcn_exp2f((u * u) * -0.72134752044448170f);
  float q = -0.30087511512911436f;
  q = fmaf(q, s, 0.4339584527532372f);
  q = fmaf(q, s, 0.8220608039774832f);
  q = fmaf(q, s, -3.070689406167805f);
  q = fmaf(q, s, 4.114633908437599f);
  q = fmaf(q, s, -3.012377713453634f);
  q = fmaf(q, s, 1.0f);
  return fmaf(-q, gauss, 1.0f);
}
__device__ __forceinline__ float vr_gelu(float x) {        // 0.5 x (1 + erf(x / sqrt 2)) = 0.5 x + 0.5 |x| erf(|x| / sqrt 2)
  float g;
  const float e = vr_erf_abs(x, g);
  return fmaf(0.5f * fabsf(x), e, 0.5f * x);
}
// gelu(x) and gelu'(x) = cdf + x pdf from one erf evaluation
__device__ __forceinline__ float vr_gelu_both(float x, float& grad) {
  float g;
  const float e = vr_erf_abs(x, g);
  const float cdf = 0.5f + copysignf(0.5f * e, x);
  grad = fmaf(x, 0.39894228040143268f * g, cdf);
  return x * cdf;
}
__device__ __forceinline__ float vr_gelu_grad(float x) {
  float grad;
  vr_gelu_both(x, grad);
  return grad;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
