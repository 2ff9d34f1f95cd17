// Dark-channel-prior dehazing (He et al.) of raw frames on the device: the reference's image_augmentation_test/dark_channel.py
// restated; the host statement is render.dehaze_host, and the kernels equal it bit for bit.
//
// THE RULE, for one (ih, iw, 3) uint8 RGB image; every float64 operation is rounded on its own, in the order written
// (nothing is contracted, divisions are IEEE):
//   I_c     = double(byte_c) / 255.0
//   d8      = min over c of byte_c;  dark8 = the minimum of d8 over the sz x sz window centred on the pixel (sz odd),
//             positions outside the image ignored (cv2.erode's default border); uint8
//   numpx   = max(ih iw / 1000, 1) (integer division).  The pixels in ascending order of (dark8, flat index y iw + x): the
//             last numpx of them without the first of those; S_c = the integer sum of byte_c over these numpx - 1 pixels;
//             A_c = (double(S_c) / 255.0) / double(numpx)
//   m       = min over c of (I_c / A_c);  te = 1.0 - omega * (the same windowed minimum of m)
//   g8      = (4899 R + 9617 G + 1868 B + 8192) >> 14;  g = double(g8) / 255.0
//   box(p)  : anchor o = r / 2, refl(i, n) = |i| if |i| < n else 2 (n - 1) - |i| (REFLECT_101);
//             h(y, x) = p(y, refl(x - o, iw)), then += p(y, refl(x - o + j, iw)) for j = 1 .. r - 1 in that order; the same
//             over the rows of h; then / double(r r)
//   mI = box(g), mp = box(te), mIp = box(g * te), mII = box(g * g)
//   a = (mIp - mI * mp) / ((mII - mI * mI) + eps);  b = mp - a * mI;  t = box(a) * g + box(b)
//   J_c = (I_c - A_c) / max(t, tx) + A_c;  v = J_c * 255.0;  byte = clip(rint(v), 0, 255), half to even
// DEGENERATE: any A_c == 0 (numpx == 1 included: nothing is summed), or r / 2 > min(ih, iw) - 1 (no single reflection).
// Such an image comes back unchanged with t = 1 and sets VR_FLAG_DEHAZE.  A geometry record with ih, iw <= 0 or above the
// slot sets VR_FLAG_GEOMETRY and gives a zero image.  Outside an image's corner of its slot out and transmission are 0.
//
// THE LAUNCHES (one body each for fixed-size batches and geometry tables):
//   dh_init          per image: the size from the table, the record, the histogram and the sums zeroed
//   dh_erode<u8>     32 x 16 tiles with a halo of sz / 2 in LDS, separable minimum (a minimum has no order): dark8, and the
//                    image's 256-bin histogram (LDS atomics, then one global integer atomic per non-empty bin)
//   dh_threshold     per image: the threshold bin T (the highest with numpx or more pixels at or above it), how many of
//                    its pixels are taken (numpx - #above - 1, the one dropped being the lowest index taken) and its size
//   dh_count         per chunk of 4096 flat indices: the pixels of bin T
//   dh_sum           per chunk: the bin-T pixels before it (the sum of the earlier chunks' counts), each bin-T pixel's
//                    rank through a workgroup prefix sum, S_c of the taken pixels in 64-bit integer atomics
//   dh_finish        per image: A, the degenerate decision, the flag; the record the later launches read wave-uniformly
//   dh_erode<f64>    m (from a 768-entry table of I_c / A_c per tile: the same divisions, once per byte value) and its
//                    windowed minimum, te
//   dh_box_h<0>      rows of g (recomputed from the bytes) and te in LDS; the horizontal sums of g, te, g te, g g
//   dh_box_v<0>      columns through an LDS tile of 32 columns x (32 + r - 1) rows, plane by plane; a and b
//   dh_box_h<1>      the horizontal sums of a and b
//   dh_box_v<1>      the vertical sums, t, the recovery and the byte store; this launch covers the whole slot and also
//                    writes the zeros outside the corner and the unchanged degenerate images
// Every output's taps are added in the fixed order above by one thread; several outputs per thread give independent chains.
// Integer atomics only: the same bytes on every run.  No allocation, no memset node, no host synchronisation.
//
// WORKSPACE (vrnet_dehaze_workspace_bytes): B records of 4 doubles (A_r, A_g, A_b, 1.0 if degenerate or bad else 0.0) at
// its start -- the caller may read A there --, then the integer records, histograms, sums and chunk counts, dark8, and seven
// float64 planes of B ihm iwm: te, four horizontal sums (the first two reused for a and b's), a, b.
#include "common.h"
#include "wgscan.h"

#include <climits>

#pragma clang fp contract(off)

namespace {

constexpr int DH_MAXSZ = 31, DH_MAXR = 128;
constexpr int DH_ETW = 32, DH_ETH = 16;                       // the erosion's tile
constexpr int DH_EHALO = DH_MAXSZ / 2;
constexpr int DH_ESW = DH_ETW + 2 * DH_EHALO, DH_ESH = DH_ETH + 2 * DH_EHALO;
constexpr int DH_CHUNK = 4096, DH_PER_THREAD = 16;            // flat indices per workgroup / thread of the selection
constexpr int DH_HTW = 256, DH_HROWS = 4, DH_HK = 4;          // horizontal pass: 64 lanes x 4 outputs, a row per wave
constexpr int DH_HSEG = DH_HTW + DH_MAXR;                     // >= DH_HTW + r - 1
constexpr int DH_VTW = 32, DH_VTH = 32, DH_VK = 4;            // vertical pass: 32 columns x 8 row groups x 4 outputs
constexpr int DH_VSROWS = DH_VTH + DH_MAXR - 1;
constexpr int DH_BAD = 1, DH_DEGENERATE = 2;                  // bits of DhRec::state

struct DhRec {                      // the integer record of one image
  int state, ih, iw, T;             // T: the threshold bin
  int first, cT, numpx, pad;        // first: the rank within bin T (ascending flat index) of the first pixel taken
};

struct DhArgs {
  const unsigned char* frames;      // (B, ihm, iwm, 3)
  const vrnet_frame_geom* geom;     // (B) or NULL
  unsigned char* out;               // (B, ihm, iwm, 3)
  double* trans;                    // (B, ihm, iwm) or NULL
  int* flag;
  double* recd;                     // (B, 4)
  DhRec* rec;                       // (B)
  int* hist;                        // (B, 256)
  unsigned long long* sums;         // (B, 4)
  int* cnt;                         // (B, nchunks)
  unsigned char* dark;              // (B, ihm, iwm)
  double* te;                       // the planes, (B, ihm, iwm) each
  double* h[4];
  double* pa;
  double* pb;
  double eps, omega, tx;
  int B, ihm, iwm, sz, r, nchunks;
};

__device__ __forceinline__ int dh_refl(int i, int n) {
  i = i < 0 ? -i : i;
  return i < n ? i : 2 * (n - 1) - i;
}
__device__ __forceinline__ int dh_gray(const unsigned char* px) {
  return (4899 * (int)px[0] + 9617 * (int)px[1] + 1868 * (int)px[2] + 8192) >> 14;
}

__global__ __launch_bounds__(256) void dh_init_kernel(const DhArgs p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  p.hist[b * 256 + tid] = 0;
  if (tid < 4) p.sums[b * 4 + tid] = 0ull;
  if (tid == 0) {
    int ih, iw;
    bool bad;
    vr_image_size(p.geom, b, p.ihm, p.iwm, p.ihm, p.iwm, ih, iw, bad);
    int state = 0;
    if (bad) {
      state = DH_BAD;
      ih = iw = 0;
    } else if (p.r / 2 > min(ih, iw) - 1) {
      state = DH_DEGENERATE;
    }
    p.rec[b] = DhRec{state, ih, iw, 0, 0, 0, 1, 0};
  }
}

// The windowed minimum.  T = unsigned char: the source is min over c of the bytes, the result dark8 and its histogram;
// T = double: the source is min over c of (I_c / A_c), the result te = 1 - omega * minimum.
template <typename T>
__global__ __launch_bounds__(256) void dh_erode_kernel(const DhArgs p) {
  constexpr bool BYTES = sizeof(T) == 1;
  __shared__ T s_src[DH_ESH][DH_ESW];
  __shared__ T s_row[DH_ESH][DH_ETW];
  __shared__ int s_hist[BYTES ? 256 : 1];
  __shared__ double s_quot[BYTES ? 1 : 768];          // (double(v) / 255.0) / A_c for every byte v: the divisions once per tile
  const int b = blockIdx.z, tid = threadIdx.x;
  const DhRec rec = p.rec[b];
  const int x0 = blockIdx.x * DH_ETW, y0 = blockIdx.y * DH_ETH;
  if ((rec.state & DH_BAD) || (!BYTES && rec.state) || x0 >= rec.iw || y0 >= rec.ih) return;      // workgroup-uniform
  const int ih = rec.ih, iw = rec.iw, hl = p.sz / 2, sw = DH_ETW + 2 * hl, sh = DH_ETH + 2 * hl;
  const unsigned char* frame = p.frames + 3L * b * p.ihm * p.iwm;
  if constexpr (BYTES) {
    s_hist[tid] = 0;
  } else {
    for (int i = tid; i < 768; i += 256) {
      const double I = (double)(i & 255) / 255.0;
      s_quot[i] = I / p.recd[b * 4 + (i >> 8)];
    }
    __syncthreads();
  }
  for (int i = tid; i < sw * sh; i += 256) {
    const int ly = i / sw, lx = i - ly * sw, y = y0 - hl + ly, x = x0 - hl + lx;
    T v;
    if constexpr (BYTES) v = (T)255; else v = (T)__builtin_huge_val();
    if (y >= 0 && y < ih && x >= 0 && x < iw) {
      const unsigned char* px = frame + 3L * ((long)y * p.iwm + x);
      if constexpr (BYTES) {
        v = (T)min(min((int)px[0], (int)px[1]), (int)px[2]);
      } else {
        const double q0 = s_quot[px[0]], q1 = s_quot[256 + px[1]], q2 = s_quot[512 + px[2]];
        double m = q0 < q1 ? q0 : q1;
        m = m < q2 ? m : q2;
        v = (T)m;
      }
    }
    s_src[ly][lx] = v;
  }
  __syncthreads();
  for (int i = tid; i < sh * DH_ETW; i += 256) {
    const int ly = i / DH_ETW, lx = i - ly * DH_ETW;
    T m = s_src[ly][lx];
    for (int j = 1; j < p.sz; ++j) {
      const T v = s_src[ly][lx + j];
      m = v < m ? v : m;
    }
    s_row[ly][lx] = m;
  }
  __syncthreads();
  for (int i = tid; i < DH_ETH * DH_ETW; i += 256) {
    const int ly = i / DH_ETW, lx = i - ly * DH_ETW, y = y0 + ly, x = x0 + lx;
    if (y < ih && x < iw) {
      T m = s_row[ly][lx];
      for (int j = 1; j < p.sz; ++j) {
        const T v = s_row[ly + j][lx];
        m = v < m ? v : m;
      }
      const long at = ((long)b * p.ihm + y) * p.iwm + x;
      if constexpr (BYTES) {
        p.dark[at] = (unsigned char)m;
        atomicAdd(&s_hist[(int)m], 1);
      } else {
        const double e = p.omega * (double)m;
        p.te[at] = 1.0 - e;
      }
    }
  }
  if constexpr (BYTES) {
    __syncthreads();
    const int c = s_hist[tid];
    if (c) atomicAdd(&p.hist[b * 256 + tid], c);
  }
}

__global__ __launch_bounds__(64) void dh_threshold_kernel(const DhArgs p) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= p.B) return;
  DhRec rec = p.rec[b];
  if (rec.state & DH_BAD) return;
  const long n = (long)rec.ih * rec.iw;
  const long numpx = max(n / 1000, 1L);
  long above = 0;                                  // pixels in the bins above T
  int T = 255;
  for (; T > 0; --T) {
    const int c = p.hist[b * 256 + T];
    if (above + c >= numpx) break;
    above += c;
  }
  const int cT = p.hist[b * 256 + T];
  const long take = numpx - above - 1;             // of bin T, the highest flat indices; >= 0 as the histogram holds n pixels
  rec.T = T;
  rec.cT = cT;
  rec.first = (int)max(0L, min((long)cT, (long)cT - take));
  rec.numpx = (int)numpx;
  p.rec[b] = rec;
}

// the 16 consecutive flat indices of a thread; dark8 of flat index f sits at row f / iw, column f % iw of the slot
__global__ __launch_bounds__(256) void dh_count_kernel(const DhArgs p) {
  __shared__ int s_wave[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const DhRec rec = p.rec[b];
  if (rec.state & DH_BAD) return;
  const long n = (long)rec.ih * rec.iw, f0 = (long)blockIdx.x * DH_CHUNK + (long)tid * DH_PER_THREAD;
  const unsigned char* dark = p.dark + (long)b * p.ihm * p.iwm;
  int c = 0;
  if (f0 < n) {
    int y = (int)(f0 / rec.iw), x = (int)(f0 - (long)y * rec.iw);
    for (int k = 0; k < DH_PER_THREAD && f0 + k < n; ++k) {
      c += dark[(long)y * p.iwm + x] == rec.T;
      if (++x == rec.iw) {
        x = 0;
        ++y;
      }
    }
  }
  c = vr_block_sum(c, s_wave);
  if (tid == 0) p.cnt[(long)b * p.nchunks + blockIdx.x] = c;
}

__global__ __launch_bounds__(256) void dh_sum_kernel(const DhArgs p) {
  __shared__ int s_wave[4];
  __shared__ int s_scan[4];
  __shared__ unsigned int s_sum[3];
  const int b = blockIdx.y, tid = threadIdx.x;
  const DhRec rec = p.rec[b];
  if (rec.state & DH_BAD) return;
  const long n = (long)rec.ih * rec.iw, c0 = (long)blockIdx.x * DH_CHUNK;
  if (c0 >= n) return;
  // the bin-T pixels of the earlier chunks
  int before = 0;
  for (int i = tid; i < (int)blockIdx.x; i += 256) before += p.cnt[(long)b * p.nchunks + i];
  if (tid < 3) s_sum[tid] = 0u;
  before = vr_block_sum(before, s_wave);            // its barrier also stands behind the zeros of s_sum
  const long f0 = c0 + (long)tid * DH_PER_THREAD;
  const unsigned char* dark = p.dark + (long)b * p.ihm * p.iwm;
  const unsigned char* frame = p.frames + 3L * b * p.ihm * p.iwm;
  int y = 0, x = 0, mine = 0;
  if (f0 < n) {
    y = (int)(f0 / rec.iw);
    x = (int)(f0 - (long)y * rec.iw);
    int yy = y, xx = x;
    for (int k = 0; k < DH_PER_THREAD && f0 + k < n; ++k) {
      mine += dark[(long)yy * p.iwm + xx] == rec.T;
      if (++xx == rec.iw) {
        xx = 0;
        ++yy;
      }
    }
  }
  int total;                                        // the inclusive prefix over the workgroup, thread order
  int rank = before + vr_block_scan_incl<vr_op_sum>(mine, s_scan, total) - mine;      // of this thread's first bin-T pixel
  unsigned int s0 = 0, s1 = 0, s2 = 0;
  if (f0 < n) {
    for (int k = 0; k < DH_PER_THREAD && f0 + k < n; ++k) {
      const int d = dark[(long)y * p.iwm + x];
      bool taken = d > rec.T;
      if (d == rec.T) {
        taken = rank >= rec.first;
        ++rank;
      }
      if (taken) {
        const unsigned char* px = frame + 3L * ((long)y * p.iwm + x);
        s0 += px[0];
        s1 += px[1];
        s2 += px[2];
      }
      if (++x == rec.iw) {
        x = 0;
        ++y;
      }
    }
  }
  if (s0 | s1 | s2) {
    atomicAdd(&s_sum[0], s0);
    atomicAdd(&s_sum[1], s1);
    atomicAdd(&s_sum[2], s2);
  }
  __syncthreads();
  if (tid < 3 && s_sum[tid]) atomicAdd(&p.sums[b * 4 + tid], (unsigned long long)s_sum[tid]);
}

__global__ __launch_bounds__(64) void dh_finish_kernel(const DhArgs p) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= p.B) return;
  DhRec rec = p.rec[b];
  double A[3] = {0.0, 0.0, 0.0};
  if (!(rec.state & DH_BAD)) {
    for (int c = 0; c < 3; ++c) {
      const double s = (double)(long long)p.sums[b * 4 + c] / 255.0;
      A[c] = s / (double)rec.numpx;
    }
    if (A[0] == 0.0 || A[1] == 0.0 || A[2] == 0.0) rec.state |= DH_DEGENERATE;
  }
  p.rec[b].state = rec.state;
  p.recd[b * 4] = A[0];
  p.recd[b * 4 + 1] = A[1];
  p.recd[b * 4 + 2] = A[2];
  p.recd[b * 4 + 3] = rec.state ? 1.0 : 0.0;
  if (p.flag && rec.state)
    atomicOr(p.flag, (rec.state & DH_BAD) ? VR_FLAG_GEOMETRY : VR_FLAG_DEHAZE);
}

// The horizontal pass.  MODE 0: u = g (from the bytes), v = te; sums of u, v, u v, u u into h[0..3].  MODE 1: u = a, v = b;
// sums into h[0], h[1].  A wave owns a row; lane l owns the outputs x0 + l + 64 k.
template <int MODE>
__global__ __launch_bounds__(256) void dh_box_h_kernel(const DhArgs p) {
  __shared__ double s_u[DH_HROWS][DH_HSEG];
  __shared__ double s_v[DH_HROWS][DH_HSEG];
  const int b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const DhRec rec = p.rec[b];
  const int x0 = blockIdx.x * DH_HTW, y = blockIdx.y * DH_HROWS + wave;
  if (rec.state || x0 >= rec.iw || (int)blockIdx.y * DH_HROWS >= rec.ih) return;              // workgroup-uniform
  const int iw = rec.iw, r = p.r, o = r / 2, nout = min(DH_HTW, iw - x0);
  const bool row = y < rec.ih;                                                                // wave-uniform
  const long base = ((long)b * p.ihm + y) * p.iwm;
  if (row) {
    for (int e = lane; e < nout + r - 1; e += 64) {
      const int xs = dh_refl(x0 - o + e, iw);
      if (MODE == 0) {
        const double g8 = (double)dh_gray(p.frames + 3L * (base + xs));
        s_u[wave][e] = g8 / 255.0;
        s_v[wave][e] = p.te[base + xs];
      } else {
        s_u[wave][e] = p.pa[base + xs];
        s_v[wave][e] = p.pb[base + xs];
      }
    }
  }
  __syncthreads();
  if (!row) return;
  double su[DH_HK], sv[DH_HK], suv[DH_HK], suu[DH_HK];
#pragma unroll
  for (int k = 0; k < DH_HK; ++k) {
    const double u = s_u[wave][lane + 64 * k], v = s_v[wave][lane + 64 * k];
    su[k] = u;
    sv[k] = v;
    if (MODE == 0) {
      suv[k] = u * v;
      suu[k] = u * u;
    }
  }
  for (int j = 1; j < r; ++j) {
#pragma unroll
    for (int k = 0; k < DH_HK; ++k) {                 // lane + 64 k + j <= 63 + 192 + 127: inside the segment
      const double u = s_u[wave][lane + 64 * k + j], v = s_v[wave][lane + 64 * k + j];
      su[k] += u;
      sv[k] += v;
      if (MODE == 0) {
        const double uv = u * v, uu = u * u;
        suv[k] += uv;
        suu[k] += uu;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < DH_HK; ++k) {
    const int xo = lane + 64 * k;
    if (xo < nout) {
      p.h[0][base + x0 + xo] = su[k];
      p.h[1][base + x0 + xo] = sv[k];
      if (MODE == 0) {
        p.h[2][base + x0 + xo] = suv[k];
        p.h[3][base + x0 + xo] = suu[k];
      }
    }
  }
}

// The vertical pass over the slot in 32 x 32 tiles: thread (cx, ry) owns the outputs (y0 + ry + 8 k, x0 + cx).
// MODE 0: the four sums -> a, b.  MODE 1: the two sums -> t, the recovery, out and transmission; everything else of the slot.
template <int MODE>
__global__ __launch_bounds__(256) void dh_box_v_kernel(const DhArgs p) {
  constexpr int NP = MODE == 0 ? 4 : 2;
  __shared__ double s_t[DH_VSROWS][DH_VTW];
  const int b = blockIdx.z, cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
  const DhRec rec = p.rec[b];
  const int x0 = blockIdx.x * DH_VTW, y0 = blockIdx.y * DH_VTH, x = x0 + cx;
  const bool work = rec.state == 0 && x0 < rec.iw && y0 < rec.ih;                            // workgroup-uniform
  if (MODE == 0 && !work) return;
  const int ih = rec.ih, iw = rec.iw, r = p.r, o = r / 2;
  const long slot = (long)b * p.ihm * p.iwm;
  double acc[NP][DH_VK];
  if (work) {
    const int nrow = min(DH_VTH, ih - y0);
    for (int q = 0; q < NP; ++q) {
      const double* src = p.h[q] + slot;
      for (int i = threadIdx.x; i < (nrow + r - 1) * DH_VTW; i += 256) {
        const int e = i >> 5, c = i & 31;
        if (x0 + c < iw) s_t[e][c] = src[(long)dh_refl(y0 - o + e, ih) * p.iwm + x0 + c];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < DH_VK; ++k) acc[q][k] = s_t[ry + 8 * k][cx];
      for (int j = 1; j < r; ++j) {
#pragma unroll
        for (int k = 0; k < DH_VK; ++k) acc[q][k] += s_t[ry + 8 * k + j][cx];      // ry + 8 k + j <= 31 + 127: inside the tile
      }
      __syncthreads();
    }
  }
  const double rr = (double)(r * r);
#pragma unroll
  for (int k = 0; k < DH_VK; ++k) {
    const int y = y0 + ry + 8 * k;
    const long at = slot + (long)y * p.iwm + x;
    if constexpr (MODE == 0) {
      if (y < ih && x < iw) {
        const double mI = acc[0][k] / rr, mp = acc[1][k] / rr, mIp = acc[2][k] / rr, mII = acc[3][k] / rr;
        const double cov = mIp - mI * mp, var = mII - mI * mI;
        const double a = cov / (var + p.eps);
        p.pa[at] = a;
        p.pb[at] = mp - a * mI;
      }
    } else {
      if (y >= p.ihm || x >= p.iwm) continue;
      const unsigned char* px = p.frames + 3 * at;
      unsigned char* dst = p.out + 3 * at;
      double t = 0.0;
      unsigned int q0 = 0, q1 = 0, q2 = 0;
      if (y < ih && x < iw) {                           // ih = iw = 0 for a bad record
        q0 = px[0];
        q1 = px[1];
        q2 = px[2];
        t = 1.0;
        if (work) {
          const double ma = acc[0][k] / rr, mb = acc[1][k] / rr;
          const double g = (double)dh_gray(px) / 255.0;
          t = ma * g + mb;
          const double d = t > p.tx ? t : p.tx;
          const unsigned int in[3] = {q0, q1, q2};
          unsigned int res[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double A = p.recd[b * 4 + c];
            const double J = ((double)in[c] / 255.0 - A) / d + A;
            double v = __builtin_rint(J * 255.0);
            v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
            res[c] = (unsigned int)(int)v;
          }
          q0 = res[0];
          q1 = res[1];
          q2 = res[2];
        }
      }
      dst[0] = (unsigned char)q0;
      dst[1] = (unsigned char)q1;
      dst[2] = (unsigned char)q2;
      if (p.trans) p.trans[at] = t;
    }
  }
}

struct DhLayout {
  long recd, rec, hist, sums, cnt, dark, planes, plane, total;
  int nchunks;
};
DhLayout dh_layout(int B, int ihm, int iwm) {
  DhLayout l;
  const long px = (long)ihm * iwm;
  l.nchunks = (int)vr_cdiv(px, DH_CHUNK);
  l.recd = 0;
  l.rec = vr_align256(l.recd + 32L * B);
  l.hist = vr_align256(l.rec + (long)sizeof(DhRec) * B);
  l.sums = vr_align256(l.hist + 1024L * B);
  l.cnt = vr_align256(l.sums + 32L * B);
  l.dark = vr_align256(l.cnt + 4L * B * l.nchunks);
  l.planes = vr_align256(l.dark + (long)B * px);
  l.plane = vr_align256(8L * B * px);
  l.total = l.planes + 7 * l.plane;
  return l;
}
bool dh_shape_ok(int B, int ihm, int iwm) {
  return B > 0 && B < 65536 && ihm > 0 && iwm > 0 && ihm <= (1 << 17) && iwm <= (1 << 17) && (long)ihm * iwm <= (1L << 26) &&
         (long)B * ihm * iwm <= (1L << 31);
}

}  // namespace

extern "C" long vrnet_dehaze_workspace_bytes(int B, int ihm, int iwm) {
  if (!dh_shape_ok(B, ihm, iwm)) return -1;
  return dh_layout(B, ihm, iwm).total;
}

extern "C" int vrnet_dehaze_u8(const unsigned char* frames, const vrnet_frame_geom* geom, int B, int ihm, int iwm, int sz, int r,
                               double eps, double omega, double tx, unsigned char* out, double* transmission, int* flag,
                               void* workspace, long workspace_bytes, void* stream) {
  VR_CHECK_ARG(frames && out && workspace && frames != out, "dehaze: frames, out (a different buffer) and the workspace are required");
  VR_CHECK_ARG(dh_shape_ok(B, ihm, iwm),
               "dehaze: bad shape (B %d, slots of %d x %d; 1..65535 images, sides up to 2^17, at most 2^26 pixels each and 2^31 in all)", B, ihm, iwm);
  VR_CHECK_ARG(sz >= 1 && sz <= DH_MAXSZ && (sz & 1) && r >= 2 && r <= DH_MAXR,
               "dehaze: sz %d must be odd in 1..%d and r %d in 2..%d", sz, DH_MAXSZ, r, DH_MAXR);
  VR_CHECK_ARG(eps > 0.0 && eps < __builtin_huge_val() && omega > 0.0 && omega <= 1.0 && tx > 0.0 && tx <= 1.0,
               "dehaze: eps %g must be positive and finite, omega %g and tx %g in (0, 1]", eps, omega, tx);
  const DhLayout l = dh_layout(B, ihm, iwm);
  if (workspace_bytes < l.total) {
    vr_set_error("dehaze: the workspace holds %ld bytes, %ld are needed", workspace_bytes, l.total);
    return VR_ERR_WORKSPACE;
  }
  VR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(transmission) & 7) == 0,
               "dehaze: the workspace and transmission must be 8-byte aligned");
  char* ws = static_cast<char*>(workspace);
  DhArgs p;
  p.frames = frames;
  p.geom = geom;
  p.out = out;
  p.trans = transmission;
  p.flag = flag;
  p.recd = reinterpret_cast<double*>(ws + l.recd);
  p.rec = reinterpret_cast<DhRec*>(ws + l.rec);
  p.hist = reinterpret_cast<int*>(ws + l.hist);
  p.sums = reinterpret_cast<unsigned long long*>(ws + l.sums);
  p.cnt = reinterpret_cast<int*>(ws + l.cnt);
  p.dark = reinterpret_cast<unsigned char*>(ws + l.dark);
  double* planes[7];
  for (int i = 0; i < 7; ++i) planes[i] = reinterpret_cast<double*>(ws + l.planes + i * l.plane);
  p.te = planes[0];
  for (int i = 0; i < 4; ++i) p.h[i] = planes[1 + i];
  p.pa = planes[5];
  p.pb = planes[6];
  p.eps = eps;
  p.omega = omega;
  p.tx = tx;
  p.B = B;
  p.ihm = ihm;
  p.iwm = iwm;
  p.sz = sz;
  p.r = r;
  p.nchunks = l.nchunks;
  hipStream_t st = vr_stream(stream);
  const dim3 per_image((unsigned int)vr_cdiv(B, 64)), chunks(l.nchunks, B);
  const dim3 etiles((unsigned int)vr_cdiv(iwm, DH_ETW), (unsigned int)vr_cdiv(ihm, DH_ETH), B);
  const dim3 htiles((unsigned int)vr_cdiv(iwm, DH_HTW), (unsigned int)vr_cdiv(ihm, DH_HROWS), B);
  const dim3 vtiles((unsigned int)vr_cdiv(iwm, DH_VTW), (unsigned int)vr_cdiv(ihm, DH_VTH), B);
  hipLaunchKernelGGL(dh_init_kernel, dim3(B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("dehaze (init)");
  hipLaunchKernelGGL(dh_erode_kernel<unsigned char>, etiles, dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("dehaze (dark channel)");
  hipLaunchKernelGGL(dh_threshold_kernel, per_image, dim3(64), 0, st, p);
  VR_LAUNCH_CHECK("dehaze (threshold)");
  hipLaunchKernelGGL(dh_count_kernel, chunks, dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("dehaze (count)");
  hipLaunchKernelGGL(dh_sum_kernel, chunks, dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("dehaze (sum)");
  hipLaunchKernelGGL(dh_finish_kernel, per_image, dim3(64), 0, st, p);
  VR_LAUNCH_CHECK("dehaze (atmospheric light)");
  hipLaunchKernelGGL(dh_erode_kernel<double>, etiles, dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("dehaze (transmission estimate)");
  hipLaunchKernelGGL(dh_box_h_kernel<0>, htiles, dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("dehaze (box rows)");
  hipLaunchKernelGGL(dh_box_v_kernel<0>, vtiles, dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("dehaze (box columns, a and b)");
  hipLaunchKernelGGL(dh_box_h_kernel<1>, htiles, dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("dehaze (box rows of a and b)");
  hipLaunchKernelGGL(dh_box_v_kernel<1>, vtiles, dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("dehaze (recovery)");
  return VR_OK;
}
