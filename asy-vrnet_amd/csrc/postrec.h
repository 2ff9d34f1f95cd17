// The per-image record of the blur and the rotation (data.AUG_POST_DTYPE) and how a kernel judges it, shared by the post
// kernels of the augmentation (csrc/augment.hip) and the radar map from points under a rotation (csrc/radarmap.hip): both must
// call the same records bad, so the rule is written here once.
#pragma once
#include "common.h"

extern "C" {
/* include/vrnet_hip.h: the per-image record of the blur and the rotation (112 bytes). */
typedef struct vrnet_aug_post_rec {
  int blur, rotate;                  /* != 0: blur the canvas; rotate canvas, label map, radar map and boxes */
  int angle, reserved;               /* the reference's `rotation` in degrees, judged against max_angle */
  double inv[6], fwd[6];             /* data.rotation_matrices: the map warpAffine walks, and the one the boxes take */
} vrnet_aug_post_rec;
}
static_assert(sizeof(vrnet_aug_post_rec) == 112 && alignof(vrnet_aug_post_rec) == 8, "vrnet_aug_post_rec layout");

struct PostRec {
  int blur, rotate;
  double inv[6], fwd[6];
};

// Record b, judged: a matrix entry that is not finite, or |angle| above the capacity the caller sized the LDS region for, is
// `bad`: the record then neither blurs nor rotates (and is reported).  b is block-uniform, so the loads are wave-uniform.
__device__ __forceinline__ PostRec post_load(const vrnet_aug_post_rec* tab, int b, int max_angle, bool& bad) {
  const vrnet_aug_post_rec* t = tab + b;
  PostRec q;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    q.inv[k] = t->inv[k];
    q.fwd[k] = t->fwd[k];
    finite = finite && isfinite(q.inv[k]) && isfinite(q.fwd[k]);
  }
  const long angle = t->angle;
  bad = !finite || angle > max_angle || angle < -(long)max_angle;
  q.blur = !bad && t->blur != 0;
  q.rotate = !bad && t->rotate != 0;
  return q;
}

// what every entry point that takes a post table asks of max_angle
constexpr int POST_MAX_ANGLE = 45;
