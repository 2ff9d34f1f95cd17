// A baseline JPEG encoder: every image of a batch to a complete JFIF file in its slot of a byte arena, every byte the one
// Pillow (libjpeg-turbo) writes for Image.save(format="JPEG", quality=q, subsampling=0 or 2).
//
// THE RULE (host statement: render.jpeg_encode_host, pinned to Pillow without a GPU by tests/test_jpeg_host.py).  Integer
// arithmetic from end to end, >> arithmetic:
//   colour    Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16,
//             Cr = (32768 R - 27439 G - 5329 B + 8421375) >> 16.
//   edges     4:4:4: every plane replicated to multiples of 8, an MCU = one block each of Y, Cb, Cr.  4:2:0: MCUs of 16 x 16,
//             Y replicated; a chroma plane replicated to the EVEN height h + (h & 1) and to width 16 MW, reduced by
//             (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ... along the output columns, and the REDUCED plane
//             replicated down to 8 MH rows.  An MCU is Y(0,0), Y(0,1), Y(1,0), Y(1,1), Cb, Cr; a Y block beyond ceil(h / 8) block
//             rows or ceil(w / 8) block columns is a DUMMY: no AC, and the DC of the block in front of it.
//   DCT       libjpeg's jfdctint on samples minus 128 (CONST_BITS 13, PASS1_BITS 2): rows, then columns.
//   quantise  d = 8 t, m = (|c| + (d >> 1)) / d, the sign restored; t from the DQT segments of the header template.
//   entropy   one DC predictor per component, never reset; category = bit length of |v|, value bits = the low s bits of v
//             (of v - 1 below zero); AC as (run << 4) | s in zigzag order with ZRL and EOB; the Annex K tables; bits MSB first,
//             the last byte padded with ones, 0x00 behind every 0xFF; then EOI.
//
// EIGHT LAUNCHES, no host synchronisation, no allocation, integer atomics only (the same bytes on every run):
//   jpeg_block_kernel   8 threads a block, 32 blocks a workgroup: thread r of a block makes row r of its samples from the
//                       pixels (colour, replication, the 4:2:0 reduction), runs the row pass, the block goes through LDS
//                       (rows of 9 words: no bank conflict either way), the thread runs column r, quantises and puts the
//                       coefficients into LDS at their zigzag positions; the workgroup's 4 KiB of int16 leave in 16-byte stores.
//   jpeg_length_kernel  a wave per block, a lane per coefficient, 256 blocks a workgroup: the ballot of the non-zero lanes is
//                       the run structure (run = distance to the set bit below), a wave sum is the block's bit count; the
//                       workgroup scans its 256 counts (exclusive, `bitoff`) and leaves their sum (`chunk`).
//   jpeg_scan_kernel    a workgroup per image: the exclusive scan of the chunk sums in place, the bits of the image, and the
//                       first capacity check (the file without its stuffing bytes).
//   jpeg_zero_kernel    zeroes the words of the image's bit stream that the next kernel ORs into.
//   jpeg_emit_kernel    as the length kernel, plus a wave prefix over the lanes: every lane ORs its at most 59 bits (three
//                       ZRL, a 16-bit code, 10 value bits) into at most three 32-bit words of the stream with atomicOr.
//   jpeg_ffcount_kernel the 0xFF bytes of every 1024 bytes of the stream, the padding of the last byte applied.
//   jpeg_ffscan_kernel  a workgroup per image: the exclusive scan of those counts, the final capacity check, the record
//                       (length, state) and VR_FLAG_JPEG_ARENA.
//   jpeg_pack_kernel    every byte to 623 + its index + the 0xFF bytes in front of it, 0x00 behind a 0xFF; one more
//                       workgroup an image writes the header from the template, height and width patched, and EOI.
// BIT OFFSETS ARE 32-BIT: a block codes to at most 20 + 63 * 26 = 1658 bits and the entry point refuses slots of more than
// 2^20 blocks (JP_MAX_BLOCKS), so an image's bits stay below 2^31.
// An image whose file does not fit `capacity` gets the record (0, 2) and nothing of its slot is written by the pack kernel;
// a size record that had to be clamped sets VR_FLAG_GEOMETRY, one without pixels gives the record (0, 3).
#include "common.h"
#include "wgscan.h"

namespace {

constexpr int JP_HEADER = 623;           // bytes in front of the scan data
constexpr int JP_DQT0 = 25, JP_DQT1 = 94;    // the 64 bytes of the two quantisation tables in the header, zigzag order
constexpr int JP_SOF_SIZE = 163;         // height and width, two big-endian bytes each
constexpr int JP_MAX_BLOCKS = 1 << 20;
constexpr int JP_BLOCKS_WG = 32;         // blocks per workgroup of the block kernel
constexpr int JP_SCAN_CHUNK = 256;       // blocks per workgroup of the length and emit kernels
constexpr int JP_STUFF_CHUNK = 1024;     // bytes of the stream per workgroup of the count and pack kernels

struct JpegHuff {
  unsigned int dc[2][12];                // (length << 16) | code by category: luminance, chrominance
  unsigned int ac[2][256];               // by (run << 4) | size
  unsigned char unzig[64];               // the zigzag position of a row-major coefficient index
};

constexpr unsigned char JP_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// ITU-T T.81 Annex K.3: the code lengths 1..16 and the values of the four tables
constexpr unsigned char JP_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                             {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr unsigned char JP_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                             {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr unsigned char JP_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// T.81 Annex C: codes in order of length, counting up; the DC values are 0..11 in order
constexpr JpegHuff jpeg_make_huff() {
  JpegHuff t{};
  for (int c = 0; c < 2; ++c) {
    unsigned int code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < JP_DC_BITS[c][len - 1]; ++i) t.dc[c][k++] = ((unsigned int)len << 16) | code++;
      code <<= 1;
    }
    code = 0;
    k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < JP_AC_BITS[c][len - 1]; ++i) t.ac[c][JP_AC_VALS[c][k++]] = ((unsigned int)len << 16) | code++;
      code <<= 1;
    }
  }
  for (int z = 0; z < 64; ++z) t.unzig[JP_ZIGZAG[z]] = (unsigned char)z;
  return t;
}
__constant__ JpegHuff c_jpeg = jpeg_make_huff();

struct JpegArgs {
  const unsigned char* images;           // (B, H, W, 3)
  const vrnet_frame_geom* geom;          // (B) or NULL
  const int* sizes;                      // (B, 2) = (h, w) or NULL; neither: every image is H x W
  const unsigned char* header;           // the 623-byte template
  unsigned char* arena;                  // (B, capacity)
  int* record;                           // (B, 2) = (length, state)
  int* flag;
  short* coef;                           // (B, nbmax, 64): zigzag order, scan order
  unsigned int* bitoff;                  // (B, nbmax): a block's first bit within its chunk of JP_SCAN_CHUNK blocks
  unsigned int* chunk;                   // (B, nchunk): the bits of a chunk, then the chunk's first bit
  unsigned int* head;                    // (B, 4): bits, state (0: goes on), 0xFF bytes, 0
  unsigned int* words;                   // (B, slotwords): the bit stream, big-endian words
  unsigned int* ffc;                     // (B, nstuff): the 0xFF bytes of a chunk of the stream, then those in front of it
  long capacity;
  int B, H, W, sub, nbmax, nchunk, slotwords, nstuff;
};

// the size of image b (clamped to its slot; bad: it had to be) and its blocks
__device__ __forceinline__ void jpeg_size(const JpegArgs& p, int b, int& h, int& w, bool& bad) {
  if (p.sizes && !p.geom) vr_size_clamp(p.sizes[2 * b], p.sizes[2 * b + 1], p.H, p.W, h, w, bad);
  else vr_image_size(p.geom, b, p.H, p.W, p.H, p.W, h, w, bad);
  if (h <= 0 || w <= 0) h = w = 0;
}
__device__ __forceinline__ int jpeg_block_count(int h, int w, int sub) {
  if (h <= 0) return 0;
  return sub ? 6 * ((h + 15) >> 4) * ((w + 15) >> 4) : 3 * ((h + 7) >> 3) * ((w + 7) >> 3);
}
// whether block k of a 4:2:0 scan is a dummy Y block
__device__ __forceinline__ bool jpeg_dummy(int k, int h, int w) {
  const int mcu = k / 6, j = k - 6 * mcu;
  if (j >= 4) return false;
  const int MW = (w + 15) >> 4;
  const int by = 2 * (mcu / MW) + (j >> 1), bx = 2 * (mcu % MW) + (j & 1);
  return by >= ((h + 7) >> 3) || bx >= ((w + 7) >> 3);
}

// one pass of jfdctint over d[0..7]: first = the row pass
__device__ __forceinline__ void jpeg_fdct8(int* d, bool first) {
  const int n = first ? 11 : 15, half = 1 << (n - 1);
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = first ? (t10 + t11) << 2 : (t10 + t11 + 2) >> 2;
  d[4] = first ? (t10 - t11) << 2 : (t10 - t11 + 2) >> 2;
  int z1 = (t12 + t13) * 4433;
  d[2] = (z1 + t13 * 6270 + half) >> n;
  d[6] = (z1 - t12 * 15137 + half) >> n;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7] = (a4 + z1 + z3 + half) >> n;
  d[5] = (a5 + z2 + z4 + half) >> n;
  d[3] = (a6 + z2 + z3 + half) >> n;
  d[1] = (a7 + z1 + z4 + half) >> n;
}

__device__ __forceinline__ int jpeg_component(const unsigned char* px, int comp) {
  const int R = px[0], G = px[1], B = px[2];
  if (comp == 0) return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
  if (comp == 1) return (-11059 * R - 21709 * G + 32768 * B + 8421375) >> 16;
  return (32768 * R - 27439 * G - 5329 * B + 8421375) >> 16;
}

__global__ __launch_bounds__(256) void jpeg_block_kernel(const JpegArgs p) {
  __shared__ int s_a[256 * 9];
  __shared__ __attribute__((aligned(16))) short s_z[JP_BLOCKS_WG * 64];
  const int b = blockIdx.y, t = threadIdx.x, lb = t >> 3, r = t & 7;
  int h, w;
  bool bad;
  jpeg_size(p, b, h, w, bad);
  const int nb = jpeg_block_count(h, w, p.sub);
  if ((int)blockIdx.x * JP_BLOCKS_WG >= nb) return;                       // the whole workgroup
  const int k = blockIdx.x * JP_BLOCKS_WG + lb;
  const bool live = k < nb;
  const unsigned char* img = p.images + (long)b * p.H * p.W * 3;
  const long pitch = 3L * p.W;
  int d[8], comp = 0;
  bool zero = !live;
  if (live) {
    if (!p.sub) {
      const int mcu = k / 3, MW = (w + 7) >> 3;
      comp = k - 3 * mcu;
      const int y = min(8 * (mcu / MW) + r, h - 1), x0 = 8 * (mcu % MW);
      const unsigned char* row = img + y * pitch;
#pragma unroll
      for (int i = 0; i < 8; ++i) d[i] = jpeg_component(row + 3 * min(x0 + i, w - 1), comp) - 128;
    } else {
      const int mcu = k / 6, j = k - 6 * mcu, MW = (w + 15) >> 4;
      const int my = mcu / MW, mx = mcu % MW;
      if (j < 4) {
        const int by = 2 * my + (j >> 1), bx = 2 * mx + (j & 1);
        zero = by >= ((h + 7) >> 3) || bx >= ((w + 7) >> 3);
        if (!zero) {
          const unsigned char* row = img + min(8 * by + r, h - 1) * pitch;
#pragma unroll
          for (int i = 0; i < 8; ++i) d[i] = jpeg_component(row + 3 * min(8 * bx + i, w - 1), 0) - 128;
        }
      } else {
        comp = j - 3;
        const int cy = min(8 * my + r, ((h + 1) >> 1) - 1);               // the reduced plane, replicated downwards
        const unsigned char* ra = img + min(2 * cy, h - 1) * pitch;
        const unsigned char* rb = img + min(2 * cy + 1, h - 1) * pitch;   // the input replicated to an even height
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int cx = 8 * mx + i, xa = 3 * min(2 * cx, w - 1), xb = 3 * min(2 * cx + 1, w - 1);
          d[i] = ((jpeg_component(ra + xa, comp) + jpeg_component(ra + xb, comp) + jpeg_component(rb + xa, comp) +
                   jpeg_component(rb + xb, comp) + 1 + (cx & 1)) >> 2) - 128;
        }
      }
    }
  }
  if (zero) {
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = 0;
  }
  jpeg_fdct8(d, true);
#pragma unroll
  for (int i = 0; i < 8; ++i) s_a[t * 9 + i] = d[i];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) d[i] = s_a[lb * 72 + i * 9 + r];              // column r
  jpeg_fdct8(d, false);
  const unsigned char* qt = p.header + (comp ? JP_DQT1 : JP_DQT0);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int z = c_jpeg.unzig[8 * i + r], dv = 8 * max((int)qt[z], 1), c = d[i];
    const int m = ((c < 0 ? -c : c) + (dv >> 1)) / dv;
    s_z[lb * 64 + z] = (short)(zero ? 0 : (c < 0 ? -m : m));
  }
  __syncthreads();
  if (live)
    *reinterpret_cast<int4*>(p.coef + ((long)b * p.nbmax + k) * 64 + 8 * r) = *reinterpret_cast<const int4*>(s_z + lb * 64 + 8 * r);
}

__device__ __forceinline__ int jpeg_bitlen(int v) {
  const unsigned int a = (unsigned int)(v < 0 ? -v : v);
  return a ? 32 - __clz(a) : 0;
}
// the DC a block codes: a dummy's is that of the block in front of it (block 0 of an MCU is never a dummy)
__device__ __forceinline__ int jpeg_dc(const short* coef, int k, int h, int w, int sub) {
  if (sub)
    while (jpeg_dummy(k, h, w)) --k;
  return coef[(long)k * 64];
}
// what lane `lane` of the wave contributes to the code of block k: `len` bits, the value in the low bits of the result
__device__ __forceinline__ unsigned long long jpeg_item(const short* coef, int k, int h, int w, int sub, int lane, int& len) {
  int v = coef[(long)k * 64 + lane];
  int chroma;
  if (lane == 0) {                                                        // the DC difference to the component's predictor
    int prev = 0;
    if (!sub) {
      chroma = k % 3 != 0;
      if (k >= 3) prev = coef[(long)(k - 3) * 64];
    } else {
      const int j = k % 6;
      chroma = j >= 4;
      if (chroma) {
        if (k >= 6) prev = coef[(long)(k - 6) * 64];
      } else {
        v = jpeg_dc(coef, k, h, w, sub);
        if (j > 0) prev = jpeg_dc(coef, k - 1, h, w, sub);
        else if (k >= 6) prev = jpeg_dc(coef, k - 3, h, w, sub);          // Y(1,1) of the MCU in front
      }
    }
    v -= prev;
  } else {
    chroma = sub ? k % 6 >= 4 : k % 3 != 0;
  }
  chroma = __builtin_amdgcn_readfirstlane(chroma);
  const unsigned long long mask = __ballot(lane > 0 && v != 0);
  const int s = jpeg_bitlen(v);
  const unsigned int extra = (unsigned int)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
  len = 0;
  if (lane == 0) {
    const unsigned int e = c_jpeg.dc[chroma][min(s, 11)];
    len = (int)(e >> 16) + s;
    return ((unsigned long long)(e & 0xffffu) << s) | extra;
  }
  if (v != 0) {
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    const int run = lane - (below ? 63 - __clzll(below) : 0) - 1;
    const unsigned int e = c_jpeg.ac[chroma][((run & 15) << 4) | min(s, 10)], zrl = c_jpeg.ac[chroma][0xF0];
    unsigned long long val = ((unsigned long long)(e & 0xffffu) << s) | extra;
    len = (int)(e >> 16) + s;
    for (int n = run >> 4; n > 0; --n) {                                  // at most three
      val |= (unsigned long long)(zrl & 0xffffu) << len;
      len += (int)(zrl >> 16);
    }
    return val;
  }
  if (lane == 63) {                                                       // the block ends in zeros
    const unsigned int e = c_jpeg.ac[chroma][0];
    len = (int)(e >> 16);
    return e & 0xffffu;
  }
  return 0ull;
}

__global__ __launch_bounds__(256) void jpeg_length_kernel(const JpegArgs p) {
  __shared__ unsigned int s_wave[4];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int h, w;
  bool bad;
  jpeg_size(p, b, h, w, bad);
  const int nb = jpeg_block_count(h, w, p.sub);
  const int k0 = blockIdx.x * JP_SCAN_CHUNK;
  if (k0 >= nb) return;
  const short* coef = p.coef + (long)b * p.nbmax * 64;
  unsigned int mine = 0;
  for (int i = 0; i < 64; ++i) {
    const int k = k0 + wave * 64 + i;                                     // wave-uniform
    if (k >= nb) break;
    int len;
    jpeg_item(coef, k, h, w, p.sub, lane, len);
    const unsigned int bits = vr_wave_sum((unsigned int)len);
    if (lane == i) mine = bits;
  }
  unsigned int total;
  const unsigned int incl = vr_block_scan_incl<vr_op_sum>(mine, s_wave, total);
  const int k = k0 + threadIdx.x;
  if (k < nb) p.bitoff[(long)b * p.nbmax + k] = incl - mine;
  if (threadIdx.x == 0) p.chunk[(long)b * p.nchunk + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void jpeg_scan_kernel(const JpegArgs p) {
  __shared__ unsigned int s_wave[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  int h, w;
  bool bad;
  jpeg_size(p, b, h, w, bad);
  const int nb = jpeg_block_count(h, w, p.sub), nc = (nb + JP_SCAN_CHUNK - 1) / JP_SCAN_CHUNK;
  unsigned int* chunk = p.chunk + (long)b * p.nchunk;
  unsigned int base = 0;
  for (int c0 = 0; c0 < nc; c0 += 256) {
    const int c = c0 + tid;
    const unsigned int v = c < nc ? chunk[c] : 0u;
    unsigned int total;
    const unsigned int incl = vr_block_scan_incl<vr_op_sum>(v, s_wave, total);
    if (c < nc) chunk[c] = base + incl - v;
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    const long raw = ((long)base + 7) >> 3;
    unsigned int state = 0;
    if (nb == 0) state = 3;
    else if (JP_HEADER + raw + 2 > p.capacity || raw + 8 > 4L * p.slotwords) state = 2;
    p.head[4 * b] = base;
    p.head[4 * b + 1] = state;
    p.head[4 * b + 2] = 0;
    p.head[4 * b + 3] = 0;
  }
}

__global__ __launch_bounds__(256) void jpeg_zero_kernel(const JpegArgs p) {
  const int b = blockIdx.y;
  if (p.head[4 * b + 1]) return;
  const long n = min((long)p.slotwords, (long)(p.head[4 * b] >> 5) + 2);
  unsigned int* words = p.words + (long)b * p.slotwords;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += 256L * gridDim.x) words[i] = 0u;
}

__global__ __launch_bounds__(256) void jpeg_emit_kernel(const JpegArgs p) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (p.head[4 * b + 1]) return;
  int h, w;
  bool bad;
  jpeg_size(p, b, h, w, bad);
  const int nb = jpeg_block_count(h, w, p.sub);
  const int k0 = blockIdx.x * JP_SCAN_CHUNK;
  if (k0 >= nb) return;
  const short* coef = p.coef + (long)b * p.nbmax * 64;
  const unsigned int* bitoff = p.bitoff + (long)b * p.nbmax;
  unsigned int* words = p.words + (long)b * p.slotwords;
  const unsigned int first = p.chunk[(long)b * p.nchunk + blockIdx.x];
  for (int i = 0; i < 64; ++i) {
    const int k = k0 + wave * 64 + i;                                     // wave-uniform
    if (k >= nb) break;
    int len;
    const unsigned long long val = jpeg_item(coef, k, h, w, p.sub, lane, len);
    const unsigned int pos = first + bitoff[k] + vr_wave_scan_incl((unsigned int)len) - (unsigned int)len;
    if (len > 0) {
      const unsigned int word = pos >> 5, off = pos & 31u;
      const unsigned long long X = val << (64 - len);                     // left-aligned; len <= 59
      const unsigned long long hi = X >> off;
      const unsigned int w0 = (unsigned int)(hi >> 32), w1 = (unsigned int)hi;
      const unsigned int w2 = off ? (unsigned int)(X & ((1ull << off) - 1ull)) << (32u - off) : 0u;
      if (w0 && word < (unsigned int)p.slotwords) atomicOr(words + word, w0);
      if (w1 && word + 1 < (unsigned int)p.slotwords) atomicOr(words + word + 1, w1);
      if (w2 && word + 2 < (unsigned int)p.slotwords) atomicOr(words + word + 2, w2);
    }
  }
}

// word idx of the finished stream of `bits` bits: the padding ones of the last byte applied
__device__ __forceinline__ unsigned int jpeg_stream_word(const unsigned int* words, long idx, unsigned int bits) {
  unsigned int v = words[idx];
  const unsigned int pad = (8u - (bits & 7u)) & 7u;
  if (pad && idx == (long)(bits >> 5)) v |= ((1u << pad) - 1u) << (32u - (bits & 31u) - pad);
  return v;
}
// the 0xFF bytes among the first n (0..4) bytes of a big-endian word
__device__ __forceinline__ int jpeg_ff_bytes(unsigned int v, int n) {
  int c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) c += (j < n && ((v >> (24 - 8 * j)) & 0xffu) == 0xffu) ? 1 : 0;
  return c;
}

__global__ __launch_bounds__(256) void jpeg_ffcount_kernel(const JpegArgs p) {
  __shared__ unsigned int s_wave[4];
  const int b = blockIdx.y;
  if (p.head[4 * b + 1]) return;
  const unsigned int bits = p.head[4 * b];
  const long raw = ((long)bits + 7) >> 3;
  if ((long)blockIdx.x * JP_STUFF_CHUNK >= raw) return;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long left = raw - 4 * idx;
  unsigned int c = 0;
  if (left > 0) c = jpeg_ff_bytes(jpeg_stream_word(p.words + (long)b * p.slotwords, idx, bits), (int)min(left, 4L));
  const unsigned int total = vr_block_sum(c, s_wave);
  if (threadIdx.x == 0) p.ffc[(long)b * p.nstuff + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void jpeg_ffscan_kernel(const JpegArgs p) {
  __shared__ unsigned int s_wave[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  int h, w;
  bool bad;
  jpeg_size(p, b, h, w, bad);
  unsigned int state = p.head[4 * b + 1];
  const long raw = ((long)p.head[4 * b] + 7) >> 3;
  const int nc = state ? 0 : (int)((raw + JP_STUFF_CHUNK - 1) / JP_STUFF_CHUNK);
  unsigned int* ffc = p.ffc + (long)b * p.nstuff;
  unsigned int base = 0;
  for (int c0 = 0; c0 < nc; c0 += 256) {
    const int c = c0 + tid;
    const unsigned int v = c < nc ? ffc[c] : 0u;
    unsigned int total;
    const unsigned int incl = vr_block_scan_incl<vr_op_sum>(v, s_wave, total);
    if (c < nc) ffc[c] = base + incl - v;
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    const long length = JP_HEADER + raw + base + 2;
    if (!state && length > p.capacity) state = 2;
    p.head[4 * b + 1] = state;
    p.head[4 * b + 2] = base;
    p.record[2 * b] = state ? 0 : (int)length;
    p.record[2 * b + 1] = state ? (int)state : 1;
    if (p.flag && (state == 2 || bad)) atomicOr(p.flag, (state == 2 ? VR_FLAG_JPEG_ARENA : 0) | (bad ? VR_FLAG_GEOMETRY : 0));
  }
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const JpegArgs p) {
  __shared__ unsigned int s_wave[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (p.head[4 * b + 1]) return;
  const unsigned int bits = p.head[4 * b];
  const long raw = ((long)bits + 7) >> 3;
  unsigned char* out = p.arena + (long)b * p.capacity;                    // the ffscan kernel checked the length against capacity
  if ((int)blockIdx.x == p.nstuff) {                                      // the header and EOI
    int h, w;
    bool bad;
    jpeg_size(p, b, h, w, bad);
    for (int i = tid; i < JP_HEADER; i += 256) {
      unsigned char v = p.header[i];
      if (i == JP_SOF_SIZE) v = (unsigned char)(h >> 8);
      if (i == JP_SOF_SIZE + 1) v = (unsigned char)h;
      if (i == JP_SOF_SIZE + 2) v = (unsigned char)(w >> 8);
      if (i == JP_SOF_SIZE + 3) v = (unsigned char)w;
      out[i] = v;
    }
    if (tid < 2) out[JP_HEADER + raw + p.head[4 * b + 2] + tid] = tid ? 0xD9 : 0xFF;
    return;
  }
  if ((long)blockIdx.x * JP_STUFF_CHUNK >= raw) return;
  const long idx = (long)blockIdx.x * 256 + tid;
  const long left = raw - 4 * idx;
  const int n = left > 0 ? (int)min(left, 4L) : 0;
  const unsigned int v = n ? jpeg_stream_word(p.words + (long)b * p.slotwords, idx, bits) : 0u;
  const unsigned int c = jpeg_ff_bytes(v, n);
  unsigned int total;
  const unsigned int before = vr_block_scan_incl<vr_op_sum>(c, s_wave, total) - c + p.ffc[(long)b * p.nstuff + blockIdx.x];
  unsigned char* dst = out + JP_HEADER + 4 * idx + before;
  for (int j = 0; j < n; ++j) {
    const unsigned char byte = (unsigned char)(v >> (24 - 8 * j));
    *dst++ = byte;
    if (byte == 0xff) *dst++ = 0;
  }
}

struct JpegPlan {
  long coef, bitoff, chunk, head, words, ffc, total;                      // byte offsets into the workspace, and its size
  int nbmax, nchunk, slotwords, nstuff;
};
bool jpeg_plan(int B, int H, int W, int sub, long capacity, JpegPlan& q) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 65535 || W > 65535 || (sub != 0 && sub != 2)) return false;
  if (capacity < JP_HEADER + 2 || capacity > (1L << 31) - 64) return false;
  const long nb = sub ? 6L * ((H + 15) / 16) * ((W + 15) / 16) : 3L * ((H + 7) / 8) * ((W + 7) / 8);
  if (nb > JP_MAX_BLOCKS) return false;
  q.nbmax = (int)nb;
  q.nchunk = (int)vr_cdiv(nb, JP_SCAN_CHUNK);
  q.slotwords = (int)(vr_cdiv(capacity, 4) + 2);
  q.nstuff = (int)vr_cdiv(q.slotwords, JP_STUFF_CHUNK / 4);
  long at = 0;
  q.coef = at; at += vr_align256(2L * 64 * nb * B);
  q.bitoff = at; at += vr_align256(4L * nb * B);
  q.chunk = at; at += vr_align256(4L * q.nchunk * B);
  q.head = at; at += vr_align256(16L * B);
  q.words = at; at += vr_align256(4L * q.slotwords * B);
  q.ffc = at; at += vr_align256(4L * q.nstuff * B);
  q.total = at;
  return true;
}

}  // namespace

extern "C" long vrnet_jpeg_workspace_bytes(int B, int H, int W, int subsampling, long capacity) {
  JpegPlan q;
  return jpeg_plan(B, H, W, subsampling, capacity, q) ? q.total : -1;
}

extern "C" int vrnet_jpeg_encode_u8(const unsigned char* images, int B, int H, int W, const vrnet_frame_geom* geom, const int* sizes,
                                    int subsampling, const unsigned char* header, unsigned char* arena, long capacity, int* record,
                                    int* flag, void* ws, long ws_bytes, void* stream) {
  VR_CHECK_ARG(images && header && arena && record && ws, "jpeg_encode: images, header, arena, record and workspace are required");
  VR_CHECK_ARG(!(geom && sizes), "jpeg_encode: a geometry table or a size table, not both");
  JpegPlan q;
  VR_CHECK_ARG(jpeg_plan(B, H, W, subsampling, capacity, q),
               "jpeg_encode: bad shape (B %d, slots of %d x %d, subsampling %d, capacity %ld; 1..65535 images, sides up to 65535, "
               "at most 2^20 blocks an image, subsampling 0 or 2, capacity from 625 bytes to below 2^31)", B, H, W, subsampling, capacity);
  VR_CHECK_ARG((long)B * capacity < (1L << 40), "jpeg_encode: an arena of %ld bytes", (long)B * capacity);
  if (ws_bytes < q.total || (reinterpret_cast<uintptr_t>(ws) & 15) != 0) {
    vr_set_error("jpeg_encode: the workspace needs %ld bytes, 16-byte aligned, got %ld", q.total, ws_bytes);
    return VR_ERR_WORKSPACE;
  }
  char* base = static_cast<char*>(ws);
  const JpegArgs p{images, geom, sizes, header, arena, record, flag,
                   reinterpret_cast<short*>(base + q.coef), reinterpret_cast<unsigned int*>(base + q.bitoff),
                   reinterpret_cast<unsigned int*>(base + q.chunk), reinterpret_cast<unsigned int*>(base + q.head),
                   reinterpret_cast<unsigned int*>(base + q.words), reinterpret_cast<unsigned int*>(base + q.ffc),
                   capacity, B, H, W, subsampling, q.nbmax, q.nchunk, q.slotwords, q.nstuff};
  hipStream_t st = vr_stream(stream);
  const dim3 wg(256);
  hipLaunchKernelGGL(jpeg_block_kernel, dim3((unsigned int)vr_cdiv(q.nbmax, JP_BLOCKS_WG), B), wg, 0, st, p);
  VR_LAUNCH_CHECK("jpeg_encode (blocks)");
  hipLaunchKernelGGL(jpeg_length_kernel, dim3(q.nchunk, B), wg, 0, st, p);
  VR_LAUNCH_CHECK("jpeg_encode (lengths)");
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(B), wg, 0, st, p);
  VR_LAUNCH_CHECK("jpeg_encode (scan)");
  const unsigned int zgrid = (unsigned int)(vr_cdiv(q.slotwords, 256 * 16) < 1024 ? vr_cdiv(q.slotwords, 256 * 16) : 1024);
  hipLaunchKernelGGL(jpeg_zero_kernel, dim3(zgrid, B), wg, 0, st, p);
  VR_LAUNCH_CHECK("jpeg_encode (zero)");
  hipLaunchKernelGGL(jpeg_emit_kernel, dim3(q.nchunk, B), wg, 0, st, p);
  VR_LAUNCH_CHECK("jpeg_encode (emit)");
  hipLaunchKernelGGL(jpeg_ffcount_kernel, dim3(q.nstuff, B), wg, 0, st, p);
  VR_LAUNCH_CHECK("jpeg_encode (count)");
  hipLaunchKernelGGL(jpeg_ffscan_kernel, dim3(B), wg, 0, st, p);
  VR_LAUNCH_CHECK("jpeg_encode (stuffing scan)");
  hipLaunchKernelGGL(jpeg_pack_kernel, dim3(q.nstuff + 1, B), wg, 0, st, p);
  VR_LAUNCH_CHECK("jpeg_encode (pack)");
  return VR_OK;
}
