// The `crop` mode of detect_image, yolo.py:180-193: every kept detection cut out of the ORIGINAL frame (the reference crops
// before it draws), from the integer rows vrnet_detect_finish[_ragged]_f32 / render.box_rows make, into one packed arena.
//
// THE RULE (host statement: render.crop_boxes_host and render.crop_layout).  Row n = left, top, right, bottom, class of
// image b of size (ih, iw) is clamped again, l = max(left, 0), t = max(top, 0), r = min(right, iw), bt = min(bottom, ih),
// w = r - l, h = bt - t, so no read leaves the frame whatever the row holds.  w <= 0 or h <= 0: the crop is EMPTY, its
// record is w = h = 0 at offset 0 and nothing is copied.  Otherwise the crop is frame[t:bt, l:r, :], one contiguous
// (h, w, 3) block of the arena that begins at pixel `offset` = the sum of a over ALL earlier rows, a = w h rounded up to a
// multiple of 4 (0 for an empty row), accumulated in 64 bits: every crop starts on a 4-byte boundary, and the up to 3 pad
// pixels behind it are zero bytes.  A non-empty row with offset + a > capacity is DROPPED: its record keeps w, h and gets
// offset -1, and VR_FLAG_CROP_ARENA is set; the sum runs over all rows, so every later non-empty row is dropped too and
// what is kept is a prefix.  summary = (N, used), used = the sum of a over the kept rows; bytes from 3 used on are not written.
//
// The image of a row comes from the offsets table made monotone: c[0] = 0, c[i] = min(N, max(0, offsets[0..i])) with
// N = offsets[B] clamped to [0, n_cap], and row n belongs to the image b with c[b] <= n < c[b + 1].
//
// TWO LAUNCHES.  crop_layout_kernel, one workgroup: the images in chunks of 256 (a running maximum of the offsets), and
// inside a chunk its rows in chunks of 256 with a running 64-bit base -- a wave prefix, the wave totals through LDS, then
// the base: box_compact_slot of augment.h carrying values instead of ballots.  crop_copy_kernel, CR_XBLOCKS workgroups per
// row of the table (a one-dimensional grid of CR_XBLOCKS n_cap: the y extent of a grid ends at 65535): workgroup x of row n
// reads record n (wave-uniform), leaves at once if the row is empty or dropped, and otherwise strides over the DWORDS of the
// crop's block; every dword is stored once, by one lane, with its four bytes gathered from the frame.  It trusts the record
// for the offset alone, and checks that: l, t, w, h are derived again from the row.
#include "common.h"
#include "wgscan.h"

#include <climits>

namespace {

constexpr int CR_XBLOCKS = 8;        // workgroups per row of the copy launch (the sweep)

struct CropArgs {
  const unsigned char* frames;       // (B, ihm, iwm, 3)
  const vrnet_frame_geom* geom;      // (B) or NULL: every image is ihm x iwm
  const int* rows;                   // (n_cap, 5)
  const int* offsets;                // (B + 1)
  unsigned char* arena;              // (3 capacity) bytes
  vrnet_crop_rec* table;             // (n_cap)
  int* summary;                      // (2)
  int* flag;
  long capacity;                     // pixels
  int B, ihm, iwm, n_cap;
};

// the clamp of a row to its image: x, y = l, t; z, w = w, h (both 0 for an empty crop)
__device__ __forceinline__ int4 crop_window(const int* row, int ih, int iw) {
  const int l = vr_clampi(row[0], 0, iw), t = vr_clampi(row[1], 0, ih);      // clamped to both ends: l > iw is empty either
  const int r = vr_clampi(row[2], 0, iw), bt = vr_clampi(row[3], 0, ih);     // way, and no difference can overflow
  const int w = r - l, h = bt - t;
  return (w <= 0 || h <= 0) ? make_int4(l, t, 0, 0) : make_int4(l, t, w, h);
}

__global__ __launch_bounds__(256) void crop_layout_kernel(const CropArgs p) {
  __shared__ int s_end[256];                          // c[i + 1] of the images of this chunk
  __shared__ int s_maxw[4];
  __shared__ long long s_sumw[4];
  __shared__ unsigned long long s_used;
  const int tid = threadIdx.x;
  const int N = vr_clampi(p.offsets[p.B], 0, p.n_cap);
  if (tid == 0) s_used = 0ull;
  long long base = 0;                                 // the pixels of all rows so far: the same in every thread
  int run = max(p.offsets[0], 0);                     // the running maximum of the offsets
  int row0 = 0;                                       // c of the chunk's first image
  bool dropped = false, badgeom = false;
  for (int i0 = 0; i0 < p.B; i0 += 256) {
    const int nimg = min(256, p.B - i0);
    int chunk_max;
    const int mine = vr_block_scan_incl<vr_op_max>(tid < nimg ? p.offsets[i0 + tid + 1] : INT_MIN, s_maxw, chunk_max);
    s_end[tid] = min(N, max(run, mine));              // threads past nimg: the chunk's end
    run = max(run, chunk_max);
    __syncthreads();
    const int row1 = s_end[nimg - 1];
    for (int r0 = row0; r0 < row1; r0 += 256) {
      const int n = r0 + tid;
      const bool valid = n < row1;
      int4 q = make_int4(0, 0, 0, 0);
      int b = 0;
      if (valid) {
        int lo = 0, hi = nimg - 1;                    // the first image of the chunk whose end lies beyond n
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_end[mid] > n) hi = mid; else lo = mid + 1;
        }
        b = i0 + lo;
        int ih, iw;
        bool bad;
        vr_image_size(p.geom, b, p.ihm, p.iwm, p.ihm, p.iwm, ih, iw, bad);
        badgeom |= bad;
        q = crop_window(p.rows + 5L * n, ih, iw);
      }
      const long long a = ((long long)q.z * q.w + 3) & ~3LL;
      long long total;
      const long long off = base + vr_block_scan_incl<vr_op_sum>(a, s_sumw, total) - a;
      base += total;
      if (valid) {
        vrnet_crop_rec rec{0, q.z, q.w, b};
        if (a > 0) {
          if (off + a > p.capacity) {
            rec.offset = -1;
            dropped = true;
          } else {
            rec.offset = (int)off;
            atomicMax(&s_used, (unsigned long long)(off + a));
          }
        }
        p.table[n] = rec;
      }
      __syncthreads();                                // s_sumw is rewritten by the next chunk
    }
    row0 = row1;
    __syncthreads();                                  // s_end and s_maxw are rewritten by the next chunk
  }
  for (int n = N + tid; n < p.n_cap; n += 256) p.table[n] = vrnet_crop_rec{0, 0, 0, -1};
  __syncthreads();
  if (tid == 0) {
    p.summary[0] = N;
    p.summary[1] = (int)s_used;
  }
  if (p.flag) {
    const unsigned long long d = __ballot(dropped), g = __ballot(badgeom);
    if ((tid & 63) == 0 && (d | g)) atomicOr(p.flag, (d ? VR_FLAG_CROP_ARENA : 0) | (g ? VR_FLAG_GEOMETRY : 0));
  }
}

__global__ __launch_bounds__(256) void crop_copy_kernel(const CropArgs p, int xblocks) {
  const int n = blockIdx.x / xblocks;                 // the workgroup's row: everything up to the loop is wave-uniform
  const unsigned int slice = blockIdx.x % xblocks;
  const vrnet_crop_rec rec = p.table[n];
  if (rec.offset < 0 || rec.w <= 0 || rec.h <= 0 || rec.image < 0 || rec.image >= p.B) return;
  int ih, iw;
  bool bad;
  vr_image_size(p.geom, rec.image, p.ihm, p.iwm, p.ihm, p.iwm, ih, iw, bad);
  const int4 q = crop_window(p.rows + 5L * n, ih, iw);
  const long long a = ((long long)q.z * q.w + 3) & ~3LL;
  if (a == 0 || (long long)rec.offset + a > p.capacity) return;          // a record that is not this row's: nothing is written
  const unsigned int D = 3u * (unsigned int)q.z;      // bytes of a crop row
  const unsigned int nbytes = D * (unsigned int)q.w;  // <= 3 capacity <= 3 * 2^30
  const unsigned int ndw = (unsigned int)(a / 4 * 3);
  const unsigned char* src = p.frames + 3L * ((long)rec.image * p.ihm * p.iwm + (long)q.y * p.iwm + q.x);
  const long pitch = 3L * p.iwm;
  unsigned int* dst = reinterpret_cast<unsigned int*>(p.arena + 3L * rec.offset);
  const unsigned int step = xblocks * 256u;           // dwords; 4 step bytes = sy crop rows and sx bytes
  const unsigned int sy = (4u * step) / D, sx = (4u * step) % D;
  unsigned int d = slice * 256u + threadIdx.x;
  unsigned int y = (4u * d) / D, x = (4u * d) % D;    // byte 4 d of the crop is byte x of its row y
  for (; d < ndw; d += step) {
    const unsigned int k = 4u * d;
    unsigned int v;
    if (x + 4u <= D && k + 4u <= nbytes) {            // four bytes of one source row: the two aligned dwords that hold them
      const unsigned char* s = src + (long)y * pitch + x;
      const unsigned int sh = (unsigned int)(reinterpret_cast<uintptr_t>(s) & 3);
      const unsigned int* s4 = reinterpret_cast<const unsigned int*>(s - sh);
      const unsigned int lo = s4[0];
      const unsigned int hi = sh ? s4[1] : 0u;        // holds byte 3 of the four, so it lies in the frame's pages
      v = (unsigned int)((((unsigned long long)hi << 32) | lo) >> (8u * sh));
    } else {                                          // across two rows of the crop, or into the pad: byte by byte
      v = 0u;
      unsigned int yy = y, xx = x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (k + j < nbytes) v |= (unsigned int)src[(long)yy * pitch + xx] << (8 * j);
        if (++xx == D) {
          xx = 0;
          ++yy;
        }
      }
    }
    dst[d] = v;
    y += sy;
    x += sx;
    if (x >= D) {
      x -= D;
      ++y;
    }
  }
}

}  // namespace

extern "C" int vrnet_crop_boxes_u8(const unsigned char* frames, int B, int ihm, int iwm, const vrnet_frame_geom* geom,
                                   const int* rows, const int* offsets, int n_cap, unsigned char* arena, long capacity_px,
                                   vrnet_crop_rec* table, int* summary, int* flag, void* stream) {
  VR_CHECK_ARG(frames && rows && offsets && arena && table && summary,
               "crop_boxes: frames, rows, offsets, arena, table and summary are required");
  VR_CHECK_ARG(B > 0 && B < 65536 && ihm > 0 && iwm > 0 && (long)ihm * iwm < (1L << 31),
               "crop_boxes: bad shape (B %d, slots of %d x %d; 1..65535 images, below 2^31 pixels each)", B, ihm, iwm);
  VR_CHECK_ARG(n_cap > 0 && n_cap <= (1 << 20) && capacity_px > 0 && capacity_px <= (1L << 30),
               "crop_boxes: %d rows outside [1, 2^20] or a capacity of %ld pixels outside [1, 2^30]", n_cap, capacity_px);
  VR_CHECK_ARG((reinterpret_cast<uintptr_t>(arena) & 3) == 0 && (reinterpret_cast<uintptr_t>(table) & 3) == 0,
               "crop_boxes: the arena and the table must be 4-byte aligned");
  const CropArgs p{frames, geom, rows, offsets, arena, table, summary, flag, capacity_px, B, ihm, iwm, n_cap};
  hipLaunchKernelGGL(crop_layout_kernel, dim3(1), dim3(256), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK("crop_boxes (layout)");
  const int tuned = vr_tune("VRNET_CROP_X", CR_XBLOCKS), xblocks = tuned < 1 ? 1 : (tuned > 1024 ? 1024 : tuned);
  hipLaunchKernelGGL(crop_copy_kernel, dim3((unsigned int)xblocks * n_cap), dim3(256), 0, vr_stream(stream), p, xblocks);
  VR_LAUNCH_CHECK("crop_boxes (copy)");
  return VR_OK;
}
