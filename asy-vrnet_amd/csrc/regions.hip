// Connected regions of the class map: the join between the semantic half (one class per pixel) and the box half (one row per
// detection) of the result.  The reference has nothing like it; the rule is this project's definition.
//
// THE RULE (host statement: decode.seg_regions_host).  For one image of size (ih, iw): pixels of class `background` are
// unlabelled (background = -1: no class is).  A region is a maximal set of pixels of one class connected under
// `connectivity` (4 or 8).  A region of fewer than min_area pixels is dropped, its pixels get label 0.  The remaining n
// regions get the ids 1..n in the order of their FIRST pixel, the smallest y iw + x.  labels holds the id of every kept
// region, whatever the table's capacity; table holds one vrnet_region per id 1..min(n, max_regions), zeros behind; head =
// (n, min(n, max_regions), pixels in kept regions, non-background pixels dropped by min_area); n > max_regions sets
// VR_FLAG_REGIONS.  The link runs over the records of the table only: a row (clamped to the image, as crops.hip clamps it)
// and a region's bounding box have the integer intersection I and union U; the best partner has the largest I / U, compared
// as I1 U2 against I2 U1 in 64 bits, I > 0 required, ties to the lowest index; det of a record is that row or -1,
// box_regions of a row is that region's id or 0.  With det_to_seg a row links only with regions of class det_to_seg[class].
//
// SEVEN LAUNCHES, none of which waits for another workgroup.
//   1. rg_tile_kernel: one workgroup labels a 64 x 16 tile in LDS.  A wave is a row of the tile, so the runs of one class in
//      a row come from one ballot and start as one set each; union-find with the LDS integer atomic minimum then joins runs
//      of neighbouring rows, ONE union per pair of touching runs (at the first pixel they share; a diagonal only where
//      neither pixel beside it joins the two).  Every pixel's parent goes as a linear index y iwm + x of the slot into an
//      int32 plane, -1 for background and outside the image.  It also zeroes the area plane and the table: everything the
//      call accumulates into.
//   2. rg_merge_kernel: one thread per pixel on a tile's first row or first column unites across the tile edges and corners
//      with the lock-free atomicMin union on the plane.  A parent is never larger than its child, so the root of a finished
//      component is its smallest index, whatever the order of arrival.  `find` reads with relaxed agent-scope atomic loads:
//      a plain load may be served from a stale line of another XCD's L2.  A stale parent still is an ancestor.
//   3. rg_flatten_kernel: every pixel resolves its root (and stores it) and adds to the area at the root in a second plane;
//      the lanes of a wave that continue a run of one parent walk once, those that continue a run of one root add once, into
//      a small table of the workgroup's roots in LDS that goes out with one atomic per root and 64 x 16 tile.
//   4. rg_count_kernel: per chunk of 2048 pixels the kept roots (root and area >= min_area), their pixels and the pixels of
//      the dropped roots.
//   5. rg_rank_kernel: every chunk sums the counts of the chunks in front of it and ranks its own kept roots: the area plane
//      then holds the id at every root, 0 at a dropped one.
//   6. rg_label_kernel: every pixel writes its label; ids inside the table accumulate area, bounding box and the two 64-bit
//      coordinate sums with integer atomics, once per run of a wave into the same kind of LDS table and from there once per
//      id and tile; the root's thread writes cls, top and first.
//   7. rg_link_kernel: eight workgroups per image: both exact-fraction arg-maxima (a thread per record over the rows, which
//      pass through LDS; a wave per row over the records, reduced by shuffles), head, box_regions and the flag.
// `left` of every record starts as INT_MAX, the neutral element of its integer minimum; the last launch zeroes it behind the count.
#include "common.h"
#include "wgscan.h"

#include <climits>

namespace {

constexpr int RG_TW = 64, RG_TH = 16;      // the tile of the LDS pass: a wave per tile row
constexpr int RG_CHUNK = 2048;             // pixels per workgroup of the count and rank launches: 8 per thread

struct RegionArgs {
  const unsigned char* cls;                // (B, ihm, iwm)
  const vrnet_frame_geom* geom;            // (B) or NULL: every image is ih x iw
  const int* rows;                         // (n_cap, 5)
  const int* offsets;                      // (B + 1)
  const int* det_to_seg;                   // (n_det) or NULL
  int* labels;                             // (B, ihm, iwm)
  vrnet_region* table;                     // (B, max_regions)
  int* head;                               // (B, 4)
  int* box_regions;                        // (B, cap)
  int* flag;
  int* parent;                             // workspace: (B, ihm iwm)
  int* area;                               // workspace: (B, ihm iwm); from the rank launch on the id at every root
  int* partial;                            // workspace: (B, nchunks, 4)
  long npix;                               // ihm iwm
  int B, ihm, iwm, ih, iw, n_cap, cap, connectivity, background, min_area, max_regions, n_det, nchunks;
};

// ---- union-find in LDS ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int rg_find_lds(volatile int* lab, int x) {
  for (int q = lab[x]; q != x; q = lab[x]) x = q;
  return x;
}
__device__ __forceinline__ void rg_union_lds(int* lab, int a, int b) {
  for (;;) {
    a = rg_find_lds(lab, a);
    b = rg_find_lds(lab, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&lab[b], a);           // b was a root when read; old != b: somebody was faster, go on from there
    if (old == b) return;
    b = old;
  }
}

// ---- union-find on the plane ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int rg_find(int* par, int x) {
  for (;;) {
    const int q = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (q == x) return x;
    x = q;
  }
}
__device__ __forceinline__ void rg_union(int* par, int a, int b) {
  for (;;) {
    a = rg_find(par, a);
    b = rg_find(par, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + b, a);
    if (old == b) return;
    b = old;
  }
}

// the lanes that begin a run of equal keys in their wave, the length of the run that begins at this lane, and the lane at
// which this lane's run begins
__device__ __forceinline__ bool rg_run(int key, int& length, int& first) {
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(key, 1, 64);
  const bool start = lane == 0 || prev != key;
  const unsigned long long starts = __ballot(start);
  const unsigned long long rest = (starts >> lane) >> 1;
  length = rest ? __ffsll((long long)rest) : 64 - lane;
  first = 63 - __clzll((long long)(starts & ((2ull << lane) - 1ull)));      // lane 0 always starts a run: never empty
  return start;
}
__device__ __forceinline__ bool rg_run(int key, int& length) {
  int first;
  return rg_run(key, length, first);
}

__device__ __forceinline__ int rg_block_sum(int v, int* s_wave) {      // the sum over the 256 threads, in every thread
  __syncthreads();                                                      // s_wave may still be read from the call before
  return vr_block_sum(v, s_wave);
}

__device__ __forceinline__ int rg_wave_before(const int* cnt, int wave) {      // the counts of the waves in front of this one
  int v = 0;
  for (int w = 0; w < wave; ++w) v += cnt[w];
  return v;
}

__global__ __launch_bounds__(256) void rg_tile_kernel(const RegionArgs p) {
  __shared__ int s_cls[RG_TH * RG_TW];
  __shared__ int s_lab[RG_TH * RG_TW];
  const int b = blockIdx.z, x0 = blockIdx.x * RG_TW, y0 = blockIdx.y * RG_TH;
  const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
  {                                                   // this workgroup's share of the table: zeros, and INT_MAX for every `left`
    const long nblocks = (long)gridDim.x * gridDim.y * gridDim.z;
    const long bid = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const long words = (long)p.B * p.max_regions * (long)(sizeof(vrnet_region) / 4);
    int* t = reinterpret_cast<int*>(p.table);
    for (long i = bid * 256 + threadIdx.x; i < words; i += nblocks * 256) t[i] = i % 12 == 2 ? INT_MAX : 0;     // 2: left
  }
  int ih, iw;
  bool bad;
  vr_image_size(p.geom, b, p.ihm, p.iwm, p.ih, p.iw, ih, iw, bad);
  const unsigned char* src = p.cls + (long)b * p.npix;
  const int x = x0 + lx;
  int c[4];
  bool start[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {                       // a wave is a row of the tile: a run of one class begins as one set
    const int ly = ly0 + 4 * k, y = y0 + ly, li = ly * RG_TW + lx;
    int v = -1;
    if (x < iw && y < ih) {
      v = src[(long)y * p.iwm + x];
      if (v == p.background) v = -1;
    }
    int n, first;
    start[k] = rg_run(v, n, first);
    c[k] = v;
    s_cls[li] = v;
    s_lab[li] = v >= 0 ? ly * RG_TW + first : -1;
  }
  __syncthreads();
  const bool eight = p.connectivity == 8;
#pragma unroll
  for (int k = 0; k < 4; ++k) {                       // one union per pair of touching runs: at the first pixel they share
    const int ly = ly0 + 4 * k, li = ly * RG_TW + lx;
    if (c[k] < 0 || ly == 0) continue;
    if (s_cls[li - RG_TW] == c[k]) {
      if (start[k] || s_cls[li - RG_TW - 1] != c[k]) rg_union_lds(s_lab, li, li - RG_TW);
    } else if (eight) {                               // a diagonal counts only where neither pixel beside it joins the two
      if (lx > 0 && start[k] && s_cls[li - RG_TW - 1] == c[k]) rg_union_lds(s_lab, li, li - RG_TW - 1);
      if (lx < RG_TW - 1 && s_cls[li - RG_TW + 1] == c[k] && s_cls[li + 1] != c[k]) rg_union_lds(s_lab, li, li - RG_TW + 1);
    }
  }
  __syncthreads();
  int* par = p.parent + (long)b * p.npix;
  int* area = p.area + (long)b * p.npix;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = ly0 + 4 * k, y = y0 + ly, li = ly * RG_TW + lx;
    if (x >= p.iwm || y >= p.ihm) continue;
    int root = -1;
    if (c[k] >= 0) {
      const int r = rg_find_lds(s_lab, li);
      root = (y0 + r / RG_TW) * p.iwm + x0 + r % RG_TW;
    }
    const long i = (long)y * p.iwm + x;
    par[i] = root;
    area[i] = 0;
  }
}

// nh lines y = RG_TH, 2 RG_TH, .. of iwm pixels, then nv lines x = RG_TW, 2 RG_TW, .. of ihm pixels: one thread each
__global__ __launch_bounds__(256) void rg_merge_kernel(const RegionArgs p, int nh, int nv) {
  const int b = blockIdx.y;
  long t = (long)blockIdx.x * 256 + threadIdx.x;
  int ih, iw;
  bool bad;
  vr_image_size(p.geom, b, p.ihm, p.iwm, p.ih, p.iw, ih, iw, bad);
  const unsigned char* src = p.cls + (long)b * p.npix;
  int* par = p.parent + (long)b * p.npix;
  const bool eight = p.connectivity == 8;
  const int W = p.iwm;
  if (t < (long)nh * W) {
    const int y = ((int)(t / W) + 1) * RG_TH, x = (int)(t % W);
    if (x >= iw || y >= ih) return;
    const int i = y * W + x, c = src[i];
    if (c == p.background) return;
    // one union per pair of touching runs, as in the tile: the pixel to the left makes it when it continues both runs.  Not
    // in a tile's corner: there the left neighbour is joined by the other branch below, which in turn counts on this union.
    const bool left = x > 0 && src[i - 1] == c;
    if (src[i - W] == c) {
      if (!(left && x % RG_TW != 0 && src[i - W - 1] == c)) rg_union(par, i, i - W);
    } else if (eight) {
      if (x > 0 && !left && src[i - W - 1] == c) rg_union(par, i, i - W - 1);
      if (x + 1 < iw && src[i - W + 1] == c && src[i + 1] != c) rg_union(par, i, i - W + 1);
    }
    return;
  }
  t -= (long)nh * W;
  if (t >= (long)nv * p.ihm) return;
  const int x = ((int)(t / p.ihm) + 1) * RG_TW, y = (int)(t % p.ihm);
  if (x >= iw || y >= ih) return;
  const int i = y * W + x, c = src[i];
  if (c == p.background) return;
  const bool up = y > 0 && src[i - W] == c;
  if (src[i - 1] == c) {
    if (!(up && y % RG_TH != 0 && src[i - W - 1] == c)) rg_union(par, i, i - 1);
  } else if (eight) {                                 // left differs: the two diagonals to the left, unless up or down joins them
    if (y > 0 && !up && src[i - W - 1] == c) rg_union(par, i, i - W - 1);
    if (y + 1 < ih && src[i + W - 1] == c && src[i + W] != c) rg_union(par, i, i + W - 1);
  }
}

// The sums of a workgroup's tile, gathered in LDS before they go out: RG_SLOTS keys (0: a free slot) in an open-addressed
// table.  rg_slot: the slot of `key` (> 0), claimed on the way, or -1 when the table is full and the caller adds to global
// memory itself.  A region as large as the picture then costs one global atomic per tile and field, not one per wave.
constexpr int RG_SLOTS = 32;
__device__ __forceinline__ int rg_slot(int* s_key, int key) {
  int h = key & (RG_SLOTS - 1);
  for (int probe = 0; probe < RG_SLOTS; ++probe) {
    const int old = atomicCAS(&s_key[h], 0, key);
    if (old == 0 || old == key) return h;
    h = (h + 1) & (RG_SLOTS - 1);
  }
  return -1;
}

// a 64 x 16 tile per workgroup as in rg_tile_kernel: a wave is 64 pixels of one row, four rows a thread
__global__ __launch_bounds__(256) void rg_flatten_kernel(const RegionArgs p) {
  __shared__ int s_key[RG_SLOTS], s_area[RG_SLOTS];
  const int b = blockIdx.z, x = blockIdx.x * RG_TW + (threadIdx.x & 63), ly0 = threadIdx.x >> 6;
  int ih, iw;
  bool bad;
  vr_image_size(p.geom, b, p.ihm, p.iwm, p.ih, p.iw, ih, iw, bad);
  int* par = p.parent + (long)b * p.npix;
  int* area = p.area + (long)b * p.npix;
  if (threadIdx.x < RG_SLOTS) s_key[threadIdx.x] = s_area[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = blockIdx.y * RG_TH + ly0 + 4 * k;
    const bool inside = x < iw && y < ih;
    const int i = inside ? y * p.iwm + x : 0;
    const int t = inside ? par[i] : -1;               // the root of the pixel's tile, or what the merge made of it
    int n, first;
    const bool start = rg_run(t, n, first);
    int r = t;
    if (start && t >= 0) {                            // one walk per run of one parent; other threads store roots meanwhile:
      for (int q = __hip_atomic_load(par + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); q != r;  // any value read is
           q = __hip_atomic_load(par + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))              // an ancestor
        r = q;
      if (t != r) par[t] = r;                         // the next wave that comes through t is there in one step
    }
    r = __shfl(r, first, 64);
    if (t >= 0) par[i] = r;
    if (rg_run(r, n) && r >= 0) {
      const int slot = rg_slot(s_key, r + 1);
      if (slot >= 0) atomicAdd(&s_area[slot], n); else atomicAdd(area + r, n);
    }
  }
  __syncthreads();
  if (threadIdx.x < RG_SLOTS && s_key[threadIdx.x]) atomicAdd(area + (s_key[threadIdx.x] - 1), s_area[threadIdx.x]);
}

// the roots among this thread's 8 pixels of the chunk: bit k of `roots`, their areas in a[k] (0 where the pixel is no root)
__device__ __forceinline__ void rg_chunk_roots(const RegionArgs& p, const int* par, const int* area, long base, int* a,
                                               unsigned int& roots) {
  roots = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const long i = base + k * 256 + threadIdx.x;
    a[k] = 0;
    if (i < p.npix && par[i] == (int)i) {
      a[k] = area[i];
      roots |= 1u << k;
    }
  }
}

__global__ __launch_bounds__(256) void rg_count_kernel(const RegionArgs p) {
  __shared__ int s_wave[4];
  const int b = blockIdx.y;
  const long off = (long)b * p.npix;
  int a[8];
  unsigned int roots;
  rg_chunk_roots(p, p.parent + off, p.area + off, (long)blockIdx.x * RG_CHUNK, a, roots);
  int cnt = 0, kept = 0, dropped = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (!(roots >> k & 1u)) continue;
    if (a[k] >= p.min_area) {
      ++cnt;
      kept += a[k];
    } else {
      dropped += a[k];
    }
  }
  cnt = rg_block_sum(cnt, s_wave);
  kept = rg_block_sum(kept, s_wave);
  dropped = rg_block_sum(dropped, s_wave);
  if (threadIdx.x == 0) {
    int* out = p.partial + ((long)b * p.nchunks + blockIdx.x) * 4;
    out[0] = cnt; out[1] = kept; out[2] = dropped; out[3] = 0;
  }
}

__global__ __launch_bounds__(256) void rg_rank_kernel(const RegionArgs p) {
  __shared__ int s_wave[4];
  __shared__ int s_cnt[8][4];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long off = (long)b * p.npix;
  const int* part = p.partial + (long)b * p.nchunks * 4;
  int before = 0;
  for (int c = threadIdx.x; c < (int)blockIdx.x; c += 256) before += part[4 * c];
  before = rg_block_sum(before, s_wave);
  int a[8];
  unsigned int roots;
  const long base = (long)blockIdx.x * RG_CHUNK;
  rg_chunk_roots(p, p.parent + off, p.area + off, base, a, roots);
  unsigned long long mine[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    mine[k] = __ballot((roots >> k & 1u) && a[k] >= p.min_area);
    if (lane == 0) s_cnt[k][wave] = __popcll(mine[k]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) {                       // the order of the pixels: k, then wave, then lane
    if (roots >> k & 1u) {
      int id = 0;
      if (a[k] >= p.min_area) id = before + rg_wave_before(s_cnt[k], wave) + __popcll(mine[k] & ((1ull << lane) - 1ull)) + 1;
      p.area[off + base + k * 256 + threadIdx.x] = id;
    }
    before += s_cnt[k][0] + s_cnt[k][1] + s_cnt[k][2] + s_cnt[k][3];
  }
}

__device__ __forceinline__ void rg_record_add(vrnet_region* rec, int area, int lo, int right, int bottom,
                                              unsigned long long sx, unsigned long long sy) {
  atomicAdd(&rec->area, area);
  atomicMin(&rec->left, lo);
  atomicMax(&rec->right, right);
  atomicMax(&rec->bottom, bottom);
  atomicAdd(reinterpret_cast<unsigned long long*>(&rec->sum_x), sx);
  atomicAdd(reinterpret_cast<unsigned long long*>(&rec->sum_y), sy);
}

__global__ __launch_bounds__(256) void rg_label_kernel(const RegionArgs p) {
  __shared__ int s_key[RG_SLOTS], s_area[RG_SLOTS], s_lo[RG_SLOTS], s_right[RG_SLOTS], s_bottom[RG_SLOTS];
  __shared__ unsigned long long s_sx[RG_SLOTS], s_sy[RG_SLOTS];
  const int b = blockIdx.z, x = blockIdx.x * RG_TW + (threadIdx.x & 63), ly0 = threadIdx.x >> 6;
  int ih, iw;
  bool bad;
  vr_image_size(p.geom, b, p.ihm, p.iwm, p.ih, p.iw, ih, iw, bad);
  const long off = (long)b * p.npix;
  vrnet_region* table = p.table + (long)b * p.max_regions;
  if (threadIdx.x < RG_SLOTS) {
    s_key[threadIdx.x] = s_area[threadIdx.x] = s_right[threadIdx.x] = s_bottom[threadIdx.x] = 0;
    s_lo[threadIdx.x] = INT_MAX;
    s_sx[threadIdx.x] = s_sy[threadIdx.x] = 0ull;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = blockIdx.y * RG_TH + ly0 + 4 * k;
    const long i = (long)y * p.iwm + x;               // used only where x < iwm and y < ihm
    int id = 0, r = -1;
    if (x < iw && y < ih) {
      r = p.parent[off + i];
      if (r >= 0) id = p.area[off + r];
    }
    if (x < p.iwm && y < p.ihm) p.labels[off + i] = id;
    const int key = id >= 1 && id <= p.max_regions ? id : 0;
    int n;
    const bool start = rg_run(key, n);
    if (!key) continue;
    if (start) {
      const unsigned long long sx = (unsigned long long)n * x + (unsigned long long)n * (n - 1) / 2, sy = (unsigned long long)n * y;
      const int slot = rg_slot(s_key, key);
      if (slot >= 0) {
        atomicAdd(&s_area[slot], n);
        atomicMin(&s_lo[slot], x);
        atomicMax(&s_right[slot], x + n);
        atomicMax(&s_bottom[slot], y + 1);
        atomicAdd(&s_sx[slot], sx);
        atomicAdd(&s_sy[slot], sy);
      } else {
        rg_record_add(table + (key - 1), n, x, x + n, y + 1, sx, sy);
      }
    }
    if (r == (int)i) {                                // the first pixel of the region: the one thread that writes these
      vrnet_region* rec = table + (key - 1);
      rec->cls = p.cls[off + i];
      rec->top = y;
      rec->first = y * iw + x;
    }
  }
  __syncthreads();
  if (threadIdx.x < RG_SLOTS && s_key[threadIdx.x]) {
    const int q = threadIdx.x;
    rg_record_add(table + (s_key[q] - 1), s_area[q], s_lo[q], s_right[q], s_bottom[q], s_sx[q], s_sy[q]);
  }
}

struct RgBox { int l, t, r, b; };
__device__ __forceinline__ bool rg_better(const RgBox& a, const RgBox& q, long long& bi, long long& bu, bool have) {
  const long long w = min(a.r, q.r) - max(a.l, q.l), h = min(a.b, q.b) - max(a.t, q.t);
  if (w <= 0 || h <= 0) return false;
  const long long I = w * h;
  const long long U = (long long)(a.r - a.l) * (a.b - a.t) + (long long)(q.r - q.l) * (q.b - q.t) - I;
  if (have && I * bu <= bi * U) return false;
  bi = I; bu = U;
  return true;
}

// the row of an image as the link reads it: clamped to the image, and the seg class it may link with (-1: any; an empty row,
// and one whose class the gate does not know, is l = r = 0, which overlaps nothing)
__device__ __forceinline__ RgBox rg_row_box(const RegionArgs& p, const int* row, int ih, int iw, int& want) {
  RgBox a{vr_clampi(row[0], 0, iw), vr_clampi(row[1], 0, ih), vr_clampi(row[2], 0, iw), vr_clampi(row[3], 0, ih)};
  want = -1;
  bool open = a.r > a.l && a.b > a.t;
  if (open && p.det_to_seg) {
    if (row[4] < 0 || row[4] >= p.n_det) open = false; else want = p.det_to_seg[row[4]];
  }
  if (!open) a = RgBox{0, 0, 0, 0};
  return a;
}

// RG_LINK workgroups per image share its records and its rows; each sums the chunk counts for itself
constexpr int RG_LINK = 8;
__global__ __launch_bounds__(256) void rg_link_kernel(const RegionArgs p) {
  __shared__ int s_wave[4];
  __shared__ int s_rows[2];
  __shared__ int s_box[256][5];                       // a chunk of the image's rows: l, t, r, b, want
  const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
  int ih, iw;
  bool bad;
  vr_image_size(p.geom, b, p.ihm, p.iwm, p.ih, p.iw, ih, iw, bad);
  const int* part = p.partial + (long)b * p.nchunks * 4;
  int n = 0, kept = 0, dropped = 0;
  for (int c = tid; c < p.nchunks; c += 256) {
    n += part[4 * c]; kept += part[4 * c + 1]; dropped += part[4 * c + 2];
  }
  n = rg_block_sum(n, s_wave);
  kept = rg_block_sum(kept, s_wave);
  dropped = rg_block_sum(dropped, s_wave);
  if (tid == 0) {                                     // the offsets made monotone, as crops.hip reads them
    const int N = vr_clampi(p.offsets[p.B], 0, p.n_cap);
    int run = 0;
    for (int k = 0; k <= b; ++k) run = max(run, p.offsets[k]);
    const int c0 = min(N, run), c1 = min(N, max(run, p.offsets[b + 1]));
    s_rows[0] = c0; s_rows[1] = min(c1 - c0, p.cap);
  }
  __syncthreads();
  const int nrec = min(n, p.max_regions), row0 = s_rows[0], nrows = s_rows[1];
  vrnet_region* table = p.table + (long)b * p.max_regions;
  // a thread per record over the rows in ascending order, the rows through LDS in chunks of 256
  for (int r0 = g * 256; r0 < nrec; r0 += RG_LINK * 256) {
    const int r = r0 + tid;
    vrnet_region rec{};
    if (r < nrec) rec = table[r];
    const RgBox q{rec.left, rec.top, rec.right, rec.bottom};
    int best = -1;
    long long bi = 0, bu = 1;
    for (int k0 = 0; k0 < nrows; k0 += 256) {
      __syncthreads();                                // the chunk before is read
      if (k0 + tid < nrows) {
        int want;
        const RgBox a = rg_row_box(p, p.rows + 5L * (row0 + k0 + tid), ih, iw, want);
        s_box[tid][0] = a.l; s_box[tid][1] = a.t; s_box[tid][2] = a.r; s_box[tid][3] = a.b; s_box[tid][4] = want;
      }
      __syncthreads();
      const int m = min(256, nrows - k0);
      if (r < nrec) {
        for (int k = 0; k < m; ++k) {
          if (s_box[k][4] >= 0 && s_box[k][4] != rec.cls) continue;
          const RgBox a{s_box[k][0], s_box[k][1], s_box[k][2], s_box[k][3]};
          if (rg_better(a, q, bi, bu, best >= 0)) best = k0 + k;
        }
      }
    }
    if (r < nrec) table[r].det = best;
  }
  // a wave per row, its lanes over the records in ascending order
  for (int k0 = 4 * g; k0 < p.cap; k0 += 4 * RG_LINK) {
    const int k = k0 + (tid >> 6), lane = tid & 63;
    int best = -1;
    long long bi = 0, bu = 1;
    if (k < nrows) {                                  // wave-uniform
      int want;
      const RgBox a = rg_row_box(p, p.rows + 5L * (row0 + k), ih, iw, want);
      if (a.r > a.l) {
        for (int r = lane; r < nrec; r += 64) {
          const vrnet_region* rec = table + r;
          if (want >= 0 && rec->cls != want) continue;
          const RgBox q{rec->left, rec->top, rec->right, rec->bottom};
          if (rg_better(a, q, bi, bu, best >= 0)) best = r;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {              // the larger fraction, then the lower index
        const int ob = __shfl_xor(best, o, 64);
        const long long oi = __shfl_xor(bi, o, 64), ou = __shfl_xor(bu, o, 64);
        if (ob >= 0 && (best < 0 || oi * bu > bi * ou || (oi * bu == bi * ou && ob < best))) {
          best = ob; bi = oi; bu = ou;
        }
      }
    }
    if (lane == 0 && k < p.cap) p.box_regions[(long)b * p.cap + k] = best + 1;
  }
  // behind the records: `left` still is the neutral element of the minimum; nobody reads these
  for (int r = nrec + g * 256 + tid; r < p.max_regions; r += RG_LINK * 256) table[r].left = 0;
  if (tid == 0 && g == 0) {
    int* head = p.head + 4L * b;
    head[0] = n; head[1] = nrec; head[2] = kept; head[3] = dropped;
    const int bits = (n > p.max_regions ? VR_FLAG_REGIONS : 0) | (bad ? VR_FLAG_GEOMETRY : 0);
    if (p.flag && bits) atomicOr(p.flag, bits);
  }
}

bool rg_shape_ok(int B, int ihm, int iwm) {
  return B > 0 && B < 65536 && ihm > 0 && iwm > 0 && ihm <= (1 << 17) && iwm <= (1 << 17) && (long)ihm * iwm < (1L << 31);
}

}  // namespace

extern "C" long vrnet_seg_regions_workspace_bytes(int B, int ihm, int iwm) {
  if (!rg_shape_ok(B, ihm, iwm)) return -1;
  const long npix = (long)ihm * iwm;
  return 4 * (2 * B * npix + 4 * B * vr_cdiv(npix, RG_CHUNK));
}

extern "C" int vrnet_seg_regions_u8(const unsigned char* class_map, int B, int ihm, int iwm, const vrnet_frame_geom* geom, int ih,
                                    int iw, const int* rows, const int* offsets, int n_cap, int cap, int connectivity,
                                    int background, int min_area, int max_regions, const int* det_to_seg, int n_det, int* labels,
                                    vrnet_region* table, int* head, int* box_regions, int* flag, void* workspace,
                                    long workspace_bytes, void* stream) {
  VR_CHECK_ARG(class_map && rows && offsets && labels && table && head && box_regions && workspace,
               "seg_regions: class_map, rows, offsets, labels, table, head, box_regions and the workspace are required");
  VR_CHECK_ARG(rg_shape_ok(B, ihm, iwm),
               "seg_regions: bad shape (B %d, slots of %d x %d; 1..65535 images, sides up to 2^17, below 2^31 pixels each)", B, ihm, iwm);
  VR_CHECK_ARG(geom || (ih > 0 && ih <= ihm && iw > 0 && iw <= iwm),
               "seg_regions: an image of %d x %d does not lie in its slot of %d x %d", ih, iw, ihm, iwm);
  VR_CHECK_ARG(n_cap > 0 && n_cap <= (1 << 20) && cap > 0 && cap <= (1 << 20),
               "seg_regions: %d rows or %d rows an image outside [1, 2^20]", n_cap, cap);
  VR_CHECK_ARG((connectivity == 4 || connectivity == 8) && background >= -1 && background <= 255 && min_area >= 1 &&
                   max_regions >= 1 && max_regions <= 4096,
               "seg_regions: connectivity %d (4 or 8), background %d (-1..255), min_area %d (>= 1) or max_regions %d (1..4096)",
               connectivity, background, min_area, max_regions);
  VR_CHECK_ARG((det_to_seg != nullptr) == (n_det > 0) && n_det >= 0 && n_det <= 256,
               "seg_regions: det_to_seg comes with its length in 1..256, got %d", n_det);
  VR_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 7) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0,
               "seg_regions: the table must be 8-byte aligned and the workspace 4-byte aligned");
  const long need = vrnet_seg_regions_workspace_bytes(B, ihm, iwm);
  if (workspace_bytes < need) {
    vr_set_error("seg_regions: workspace of %ld bytes, %ld needed", workspace_bytes, need);
    return VR_ERR_WORKSPACE;
  }
  const long npix = (long)ihm * iwm;
  const int nchunks = (int)vr_cdiv(npix, RG_CHUNK);
  int* ws = static_cast<int*>(workspace);
  const RegionArgs p{class_map, geom, rows, offsets, det_to_seg, labels, table, head, box_regions, flag, ws, ws + B * npix,
                     ws + 2 * B * npix, npix, B, ihm, iwm, geom ? ihm : ih, geom ? iwm : iw, n_cap, cap, connectivity, background,
                     min_area, max_regions, n_det, nchunks};
  hipStream_t st = vr_stream(stream);
  const dim3 tiles((unsigned)vr_cdiv(iwm, RG_TW), (unsigned)vr_cdiv(ihm, RG_TH), (unsigned)B);
  hipLaunchKernelGGL(rg_tile_kernel, tiles, dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("seg_regions (tiles)");
  const int nh = (ihm - 1) / RG_TH, nv = (iwm - 1) / RG_TW;
  const long border = (long)nh * iwm + (long)nv * ihm;
  if (border > 0) {
    hipLaunchKernelGGL(rg_merge_kernel, dim3((unsigned)vr_cdiv(border, 256), (unsigned)B), dim3(256), 0, st, p, nh, nv);
    VR_LAUNCH_CHECK("seg_regions (merge)");
  }
  hipLaunchKernelGGL(rg_flatten_kernel, tiles, dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("seg_regions (flatten)");
  hipLaunchKernelGGL(rg_count_kernel, dim3((unsigned)nchunks, (unsigned)B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("seg_regions (count)");
  hipLaunchKernelGGL(rg_rank_kernel, dim3((unsigned)nchunks, (unsigned)B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("seg_regions (rank)");
  hipLaunchKernelGGL(rg_label_kernel, tiles, dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("seg_regions (labels)");
  hipLaunchKernelGGL(rg_link_kernel, dim3(RG_LINK, (unsigned)B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("seg_regions (link)");
  return VR_OK;
}
