// The caption of every detection on the rendered frame: a second tag UNDER the box with what the label atlas of labels.hip
// cannot hold -- '#<track id> <range>m <closing speed>m/s', e.g. '#17 42.5m -1.2m/s'.  A track id or a range is not one of a
// fixed set of strings, so the text is composed here from numbers that exist only on the device (the table of track.hip, the
// readout of boxradar.hip), formatted exactly in integer arithmetic, and drawn from an atlas of the 18 single glyphs of
// "0123456789.-+#m/s " (render.GlyphAtlas: Pillow's own mask of each glyph in a cell of the glyph's advance).  The reference
// has nothing like it; the rule is this project's definition, stated on the host by render.caption_strings (the text),
// render.fixed_tenths (its '{:.1f}') and render.draw_captions_host (the pixels), which these kernels equal byte for byte.
//
// THE TEXT of kept row r of image b: up to three fields, joined by one space.
//   '#<id>'     with ids, for ids[b][r] > 0, in decimal;
//   the range   '{:.1f}'.format(rng) + 'm'.  With a table: the lowest slot s of stream b with id == ids[b][r], id != 0 and
//               row == r; drawn when its range_age >= 0, rng = x[4] (also while the radar coasts).  Without a table, with
//               the readout: box_points[b][r] > 0 and rng = box_radar[b][r][1][0], the lower median.  Valid when rng is not
//               NaN, its sign bit is clear and k <= 99999 (k: the tenths, below); otherwise left out, VR_FLAG_CAPTION;
//   the speed   '{:+.1f}'.format(rate) + 'm/s', only with a table, a drawn range and rate_scale > 0: rate = v[4] * rate_scale,
//               one fp32 multiply, the sign from the sign bit.  Valid when finite and k <= 9999; otherwise left out,
//               VR_FLAG_CAPTION.
// k is the exact value of the fp32 times 10 rounded to nearest with ties to even on the exact binary value, in integers on the
// bits (what Python's format prints; -0.04 gives '-0.0'); decimal digits by integer division only.  The longest caption,
// '#2147483647 9999.9m -999.9m/s', has 29 codes; a record holds 32: words 0..7 the codes as bytes, word 8 their count, 9..11 zero.
// One workgroup of 256 per image: thread s < max_tracks publishes row -> s of its slot into an LDS array of cap <= 1024 entries
// with an integer atomic minimum -- a corrupt table still gives one answer -- and behind a barrier the threads stride over
// the rows and format.
//
// THE PICTURE.  Captions are a pass of their own over the finished picture (outlines, labels); the rows of an image are drawn
// in order.  Row i with n > 0 codes at the image's font size, W the sum of its cell widths and ch the cell height:
//   (ox, oy) = (left, bottom + 1) if bottom + ch <= ih - 1, else (left, bottom - ch);
//   it paints [ox, ox + W - 1] x [oy, oy + ch - 1], clipped, in its class colour, then its cells left to right in black,
//   v = DIV255(v * (255 - m)) as labels.hip blends.
// Text never leaves its own tag, so the final value of a pixel follows from the HIGHEST row whose tag covers it: that row's
// colour blended with that row's one cell byte at the pixel.  The grid is (pixel blocks, row, image) over each row's clipped
// tag: work follows the caption area.  A workgroup stages the tag rectangles of the image's rows in LDS (16 KiB for 1024
// rows; it reads every row's 32 codes for W) and keeps the pen positions of its OWN row only; a thread leaves a pixel that a
// higher row's tag covers, otherwise it writes colour and cell byte in one store per pixel.  No racing stores, no floating
// point, no atomics on pixels.  Rows past 1024 of an image are ignored (bit 4 of *flag), as labels.hip ignores them.  Nothing
// from the tables is trusted: counts are clamped to 32, codes to 17, cell sides to 2^14, and a record whose cell leaves the
// blob draws as an empty cell.
#include "common.h"

extern "C" {
/* include/vrnet_hip.h: one track (64 bytes), as csrc/track.hip writes it; data.TRACK_DTYPE mirrors it. */
typedef struct vrnet_track {
  int id, cls, hits, misses, row, range_age;
  float x[5], v[5];
} vrnet_track;
}
static_assert(sizeof(vrnet_track) == 64 && alignof(vrnet_track) == 4 && offsetof(vrnet_track, row) == 16 &&
                  offsetof(vrnet_track, range_age) == 20 && offsetof(vrnet_track, x) == 24 && offsetof(vrnet_track, v) == 44,
              "vrnet_track is 16 words: data.TRACK_DTYPE mirrors it");

namespace {

constexpr int CP_THREADS = 256;
constexpr int CP_MAXROWS = 1024;              // cap of the text kernel; the rows of one image the draw kernel takes (RN_MAXBOX)
constexpr int CP_MAXTRACKS = 256;             // TK_MAX_TRACKS of track.hip
constexpr int CP_MAXCOL = 256;                // RN_MAXCOL of render.hip
constexpr int CP_COORD = 1 << 29;
constexpr int CP_FLAG_BOX_ROWS = 4;           // render.hip
constexpr int CP_GLYPHS = 18;                 // "0123456789.-+#m/s "
constexpr int CP_DOT = 10, CP_MINUS = 11, CP_PLUS = 12, CP_HASH = 13, CP_M = 14, CP_SLASH = 15, CP_S = 16, CP_SPACE = 17;
constexpr int CP_CODES = 32, CP_WORDS = 12;   // codes and int32 words of a caption record
constexpr int CP_REC = 4;                     // int32 per glyph record: blob offset, cell width, cell height, 0
constexpr int CP_MAXDIM = 1 << 14;            // a cell side is clamped to this
constexpr int CP_XBLOCKS = 4;                 // workgroups per row; each strides over the row's tag
constexpr int CP_SATURATED = 2147483647;
constexpr int CP_RANGE_MAX = 99999, CP_RATE_MAX = 9999;      // tenths: 9999.9 m and 999.9 m/s

__device__ __forceinline__ unsigned int div255(unsigned int a) {
  a += 128u;
  return (a + (a >> 8)) >> 8;
}

// render.fixed_tenths: k of |x|, the exact value m 2^-sh of the fp32 times 10 rounded to nearest with ties to even, saturated
__device__ __forceinline__ int cp_tenths(float x, bool& negative) {
  const unsigned int bits = __float_as_uint(x);
  negative = (bits >> 31) != 0u;
  const int e = (int)((bits >> 23) & 255u);
  if (e == 255) return CP_SATURATED;                  // an infinity or a NaN
  const unsigned long long m = (bits & 0x7FFFFFu) | (e ? 0x800000u : 0u);
  const int sh = 150 - (e ? e : 1);
  const unsigned long long N = 10ull * m;             // below 2^28
  if (sh < 1) {
    if (sh < -31) return CP_SATURATED;
    const unsigned long long v = N << -sh;
    return v > (unsigned long long)CP_SATURATED ? CP_SATURATED : (int)v;
  }
  if (sh > 63) return 0;                              // far below half a tenth
  const unsigned long long q = N >> sh, rem = N & ((1ull << sh) - 1ull), half = 1ull << (sh - 1);
  return (int)(q + ((rem > half || (rem == half && (q & 1ull))) ? 1ull : 0ull));
}

// a caption under construction: the 32 code bytes in four registers (no indexed private array) and the count
struct Caption {
  unsigned long long w[4];
  int n;
};

__device__ __forceinline__ void cp_put(Caption& c, int code) {
  if (c.n >= CP_CODES) return;
  const unsigned long long v = (unsigned long long)code << ((c.n & 7) * 8);
  const int i = c.n >> 3;
  c.w[0] |= i == 0 ? v : 0ull;
  c.w[1] |= i == 1 ? v : 0ull;
  c.w[2] |= i == 2 ? v : 0ull;
  c.w[3] |= i == 3 ? v : 0ull;
  ++c.n;
}

__device__ __forceinline__ void cp_put_decimal(Caption& c, unsigned int v) {
  unsigned int p = 1u;
  while (v / p >= 10u) p *= 10u;                      // at most 10^9: no overflow
  for (; p; p /= 10u) {
    const unsigned int d = v / p;
    v -= d * p;
    cp_put(c, (int)d);
  }
}

__device__ __forceinline__ void cp_put_tenths(Caption& c, int k) {
  cp_put_decimal(c, (unsigned int)k / 10u);
  cp_put(c, CP_DOT);
  cp_put(c, k % 10);
}

struct TextArgs {
  const int* ids;                    // (B, cap) or null
  const int* kept;                   // (B)
  const int* offsets;                // (B + 1)
  const vrnet_track* table;          // (B, T) or null
  const int* box_points;             // (B, cap) or null
  const float* box_radar;            // (B, cap, 2, 5) or null
  int* out;                          // (n_out, 12)
  int* flag;
  float rate_scale;
  int B, cap, T, n_out;
};

__global__ __launch_bounds__(CP_THREADS) void caption_text_kernel(const TextArgs p) {
  __shared__ int s_slot[CP_MAXROWS];                  // the lowest slot of the table that names the row and carries its id
  const int b = blockIdx.x, tid = threadIdx.x;
  const int raw_kept = p.kept[b];
  const int n = vr_clampi(raw_kept, 0, p.cap);
  int bits = n != raw_kept ? VR_FLAG_BOX_COUNT : 0;
  const int* ids = p.ids ? p.ids + (long)b * p.cap : nullptr;
  const vrnet_track* table = p.table ? p.table + (long)b * p.T : nullptr;
  if (table) {                                        // the block's: uniform
    for (int i = tid; i < n; i += CP_THREADS) s_slot[i] = CP_SATURATED;
    __syncthreads();
    if (tid < p.T) {
      const int id = table[tid].id, row = table[tid].row;
      if (id != 0 && row >= 0 && row < n && ids[row] == id) atomicMin(&s_slot[row], tid);
    }
    __syncthreads();
  }
  const long base = p.offsets[b];
  for (int r = tid; r < n; r += CP_THREADS) {
    const long pos = base + r;
    if (pos < 0 || pos >= p.n_out) continue;
    Caption c{};
    const int id = ids ? ids[r] : 0;
    if (id > 0) {
      cp_put(c, CP_HASH);
      cp_put_decimal(c, (unsigned int)id);
    }
    bool have = false, want_rate = false;
    float rng = 0.f, rate = 0.f;
    if (table) {
      const int s = s_slot[r];
      if (s < p.T && table[s].range_age >= 0) {
        have = true;
        rng = table[s].x[4];
        if (p.rate_scale > 0.f) {
          want_rate = true;
          rate = table[s].v[4] * p.rate_scale;
        }
      }
    } else if (p.box_points && p.box_points[(long)b * p.cap + r] > 0) {
      have = true;
      rng = p.box_radar[((long)b * p.cap + r) * 10 + 5];      // the lower median's depth
    }
    if (have) {
      bool negative;
      const int k = cp_tenths(rng, negative);
      if (rng != rng || negative || k > CP_RANGE_MAX) {
        bits |= VR_FLAG_CAPTION;
        want_rate = false;
      } else {
        if (c.n) cp_put(c, CP_SPACE);
        cp_put_tenths(c, k);
        cp_put(c, CP_M);
      }
    }
    if (want_rate) {
      bool negative;
      const int k = cp_tenths(rate, negative);
      if (!(fabsf(rate) < INFINITY) || k > CP_RATE_MAX) {
        bits |= VR_FLAG_CAPTION;
      } else {
        if (c.n) cp_put(c, CP_SPACE);
        cp_put(c, negative ? CP_MINUS : CP_PLUS);
        cp_put_tenths(c, k);
        cp_put(c, CP_M);
        cp_put(c, CP_SLASH);
        cp_put(c, CP_S);
      }
    }
    int* o = p.out + pos * CP_WORDS;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      o[2 * w] = (int)(unsigned int)c.w[w];
      o[2 * w + 1] = (int)(unsigned int)(c.w[w] >> 32);
    }
    o[8] = c.n;
    o[9] = o[10] = o[11] = 0;
  }
  if (bits && p.flag) atomicOr(p.flag, bits);
}

struct DrawArgs {
  unsigned char* pic;                // (B, ih, iw, 3), in place
  const int* boxes;                  // (n_rows, 5)
  const int* offsets;                // (B + 1)
  const int* captions;               // (n_rows, 12)
  const unsigned char* box_palette;  // (n_box_colors, 3)
  const unsigned char* blob;         // (blob_bytes)
  const int* recs;                   // (n_sizes, 18, CP_REC)
  const int* size_tab;               // RAGGED: (B) size index of image b, -1 = no captions
  const vrnet_frame_geom* tab;       // RAGGED: (B)
  int* flag;
  long blob_bytes;
  int B, ih, iw, n_rows, n_box_colors, n_sizes, size_index;
};

__device__ __forceinline__ int cp_count(const int* rec) { return vr_clampi(rec[8], 0, CP_CODES); }
__device__ __forceinline__ int cp_code(const int* rec, int i) {
  return min((int)(((unsigned int)rec[i >> 2] >> (8 * (i & 3))) & 255u), CP_GLYPHS - 1);
}

template <bool RAGGED>
__global__ __launch_bounds__(CP_THREADS) void captions_kernel(const DrawArgs p) {
  __shared__ int4 s_tag[CP_MAXROWS];                  // x0, y0, x1, y1 inclusive, not clipped; x1 < x0: no tag
  __shared__ unsigned long long s_rel[CP_MAXROWS / 64];
  __shared__ int s_cw[CP_GLYPHS], s_gh[CP_GLYPHS], s_goff[CP_GLYPHS];      // the cells of this size; offset -1: an empty cell
  __shared__ int s_pen[CP_CODES + 1], s_code[CP_CODES], s_cnt;            // this workgroup's own row
  const int tid = threadIdx.x, r = blockIdx.y, b = blockIdx.z;
  const bool first = blockIdx.x == 0 && r == 0 && tid == 0;
  int ih = p.ih, iw = p.iw, sidx = p.size_index;
  if constexpr (RAGGED) {                             // the image's own record: the block's, so wave-uniform
    bool bad;
    const vrnet_frame_geom g = vr_geom_load(p.tab, b, p.ih, p.iw, 0, 0, bad);
    sidx = p.size_tab[b];
    if (first && (bad || sidx >= p.n_sizes) && p.flag) atomicOr(p.flag, VR_FLAG_GEOMETRY);
    ih = g.ih; iw = g.iw;
    if (sidx < 0 || sidx >= p.n_sizes) return;        // no captions for this image
  }
  int start, n;
  vr_row_range(p.offsets, b, p.n_rows, start, n);
  if (n > CP_MAXROWS) {
    if (first && p.flag) atomicOr(p.flag, CP_FLAG_BOX_ROWS);
    n = CP_MAXROWS;
  }
  if (r >= n) return;                                 // the whole workgroup
  if (tid < CP_GLYPHS) {
    const int* rec = p.recs + ((long)sidx * CP_GLYPHS + tid) * CP_REC;
    const int off = rec[0], cw = vr_clampi(rec[1], 0, CP_MAXDIM), gh = vr_clampi(rec[2], 0, CP_MAXDIM);
    s_cw[tid] = cw;
    s_gh[tid] = gh;
    s_goff[tid] = (off < 0 || (long)off + (long)cw * gh > p.blob_bytes) ? -1 : off;      // a cell outside the blob: empty
  }
  __syncthreads();
  const int ch = s_gh[0];                             // the cells of one size share one height
  for (int k = tid; k < n; k += CP_THREADS) {
    const int* rec = p.captions + (long)CP_WORDS * (start + k);
    const int cnt = cp_count(rec);
    int W = 0;
    for (int i = 0; i < cnt; ++i) W += s_cw[cp_code(rec, i)];          // at most 32 * 2^14
    const int* row = p.boxes + 5L * (start + k);
    const int left = vr_clampi(row[0], -CP_COORD, CP_COORD), bottom = vr_clampi(row[3], -CP_COORD, CP_COORD);
    const int oy = bottom + ch <= ih - 1 ? bottom + 1 : bottom - ch;
    s_tag[k] = (W > 0 && ch > 0) ? make_int4(left, oy, left + W - 1, oy + ch - 1) : make_int4(0, 0, -1, -1);
  }
  if (tid == 0) {                                     // the pen positions of this workgroup's row
    const int* rec = p.captions + (long)CP_WORDS * (start + r);
    const int cnt = cp_count(rec);
    int pen = 0;
    for (int i = 0; i < cnt; ++i) {
      const int code = cp_code(rec, i);
      s_code[i] = code;
      s_pen[i] = pen;
      pen += s_cw[code];
    }
    s_pen[cnt] = pen;
    s_cnt = cnt;
  }
  for (int w = tid; w < CP_MAXROWS / 64; w += CP_THREADS) s_rel[w] = 0ull;
  __syncthreads();
  const int4 T = s_tag[r];
  int4 R = T;
  R.x = max(R.x, 0); R.y = max(R.y, 0); R.z = min(R.z, iw - 1); R.w = min(R.w, ih - 1);
  if (R.x > R.z || R.y > R.w) return;                 // the whole workgroup: R is the row's
  // the higher rows whose tag meets R: one bit per row; only they can own a pixel of R
  for (int k = r + 1 + tid; k < n; k += CP_THREADS) {
    const int4 q = s_tag[k];
    if (q.x <= R.z && q.z >= R.x && q.y <= R.w && q.w >= R.y) atomicOr(&s_rel[k >> 6], 1ull << (k & 63));
  }
  __syncthreads();
  const int cnt = s_cnt;
  const int cls = vr_clampi(p.boxes[5L * (start + r) + 4], 0, p.n_box_colors - 1);
  const unsigned int c0 = p.box_palette[3 * cls], c1 = p.box_palette[3 * cls + 1], c2 = p.box_palette[3 * cls + 2];
  const int RW = R.z - R.x + 1;
  const long npix = (long)RW * (R.w - R.y + 1);
  unsigned char* img = p.pic + 3L * b * p.ih * p.iw;  // the slot; rows of p.iw pixels
  for (long t = (long)blockIdx.x * CP_THREADS + tid; t < npix; t += (long)gridDim.x * CP_THREADS) {
    const int y = R.y + (int)(t / RW), x = R.x + (int)(t % RW);
    bool owned = true;
    for (int w = (n - 1) >> 6; w >= (r >> 6) && owned; --w) {
      unsigned long long bits = s_rel[w];
      while (bits) {
        const int j = (w << 6) + __ffsll((long long)bits) - 1;
        bits &= bits - 1ull;
        const int4 q = s_tag[j];
        if (x >= q.x && x <= q.z && y >= q.y && y <= q.w) { owned = false; break; }
      }
    }
    if (!owned) continue;
    const int px = x - T.x, py = y - T.y;
    int i = 0;
    while (i + 1 < cnt && s_pen[i + 1] <= px) ++i;    // the cell under the pixel: s_pen[i] <= px < s_pen[i + 1]
    const int code = s_code[i], off = s_goff[code];
    unsigned int m = 0u;
    if (off >= 0 && py < s_gh[code]) m = p.blob[(long)off + (long)py * s_cw[code] + (px - s_pen[i])];
    unsigned char* o = img + 3L * ((long)y * p.iw + x);
    o[0] = (unsigned char)div255(c0 * (255u - m));
    o[1] = (unsigned char)div255(c1 * (255u - m));
    o[2] = (unsigned char)div255(c2 * (255u - m));
  }
}

int captions_check(const char* fn, const DrawArgs& p) {
  VR_CHECK_ARG(p.pic && p.B > 0 && p.B < 65536 && p.ih > 0 && p.iw > 0 && p.ih <= (1 << 24) && p.iw <= (1 << 24) &&
                   (long)p.B * p.ih * p.iw < (1L << 31),
               "%s: bad shape (B %d, %d x %d; at most 2^31 - 1 pixels in all)", fn, p.B, p.ih, p.iw);
  VR_CHECK_ARG(p.n_rows >= 0 && (p.n_rows == 0 || (p.boxes && p.offsets && p.captions && p.box_palette && p.n_box_colors > 0 &&
                                                    p.n_box_colors <= CP_MAXCOL)),
               "%s: %d rows need boxes, offsets, caption records and a box palette of 1..%d colours", fn, p.n_rows, CP_MAXCOL);
  VR_CHECK_ARG(p.recs && p.n_sizes >= 1 && p.n_sizes <= 65536 && p.blob_bytes >= 0 && p.blob_bytes < (1L << 31) &&
                   (p.blob || p.blob_bytes == 0),
               "%s: the glyph atlas needs records, 1..65536 sizes and a blob below 2 GiB", fn);
  return VR_OK;
}

template <bool RAGGED>
int captions_launch(const char* fn, const DrawArgs& p, void* stream) {
  if (p.n_rows == 0) return VR_OK;
  const int rows = p.n_rows < CP_MAXROWS ? p.n_rows : CP_MAXROWS;
  // one workgroup of row 0 always exists, so more than CP_MAXROWS rows in an image are reported
  hipLaunchKernelGGL(captions_kernel<RAGGED>, dim3(CP_XBLOCKS, rows, p.B), dim3(CP_THREADS), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK(fn);
  return VR_OK;
}

}  // namespace

extern "C" int vrnet_caption_text_f32(const int* ids, const int* kept, const int* offsets, int B, int cap, const vrnet_track* table,
                                      int max_tracks, const int* box_points, const float* box_radar, float rate_scale,
                                      int* captions_out, int n_out, int* flag, void* stream) {
  const char* who = "caption_text";
  VR_CHECK_ARG(kept && offsets && captions_out, "%s: kept, offsets and captions_out are required", who);
  VR_CHECK_ARG(B > 0 && B < 65536 && cap > 0 && cap <= CP_MAXROWS && n_out >= 0 && n_out <= (1 << 26),
               "%s: bad shape (B %d, cap %d of at most %d, %d outputs of at most 2^26)", who, B, cap, CP_MAXROWS, n_out);
  VR_CHECK_ARG((box_points == nullptr) == (box_radar == nullptr), "%s: box_points and box_radar come together or not at all", who);
  VR_CHECK_ARG(ids || box_points, "%s: needs track ids or the radar readout", who);
  VR_CHECK_ARG(!table || (ids && max_tracks > 0 && max_tracks <= CP_MAXTRACKS),
               "%s: a track table needs the track ids and max_tracks in [1, %d], got %d", who, CP_MAXTRACKS, max_tracks);
  VR_CHECK_ARG(rate_scale >= 0.f && rate_scale <= 1e6f, "%s: rate_scale must lie in [0, 1e6], got %g", who, (double)rate_scale);
  if (n_out == 0) return VR_OK;
  TextArgs p{};
  p.ids = ids; p.kept = kept; p.offsets = offsets; p.table = table; p.box_points = box_points; p.box_radar = box_radar;
  p.out = captions_out; p.flag = flag; p.rate_scale = rate_scale;
  p.B = B; p.cap = cap; p.T = table ? max_tracks : 0; p.n_out = n_out;
  hipLaunchKernelGGL(caption_text_kernel, dim3((unsigned)B), dim3(CP_THREADS), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK(who);
  return VR_OK;
}

extern "C" int vrnet_render_captions_u8(unsigned char* picture, int B, int ih, int iw, const int* boxes, const int* box_offsets,
                                        int n_rows, const unsigned char* box_palette, int n_box_colors, const int* captions,
                                        const unsigned char* blob, long blob_bytes, const int* records, int n_sizes,
                                        int size_index, int* flag, void* stream) {
  DrawArgs p{};
  p.pic = picture; p.boxes = boxes; p.offsets = box_offsets; p.captions = captions; p.box_palette = box_palette;
  p.blob = blob; p.recs = records; p.flag = flag; p.blob_bytes = blob_bytes;
  p.B = B; p.ih = ih; p.iw = iw; p.n_rows = n_rows; p.n_box_colors = n_box_colors; p.n_sizes = n_sizes; p.size_index = size_index;
  if (const int rc = captions_check("render_captions", p)) return rc;
  VR_CHECK_ARG(size_index >= 0 && size_index < n_sizes, "render_captions: size index %d outside [0, %d)", size_index, n_sizes);
  return captions_launch<false>("render_captions", p, stream);
}

extern "C" int vrnet_render_captions_ragged_u8(unsigned char* picture, const vrnet_frame_geom* geom, const int* size_index, int B,
                                               int ihm, int iwm, const int* boxes, const int* box_offsets, int n_rows,
                                               const unsigned char* box_palette, int n_box_colors, const int* captions,
                                               const unsigned char* blob, long blob_bytes, const int* records, int n_sizes,
                                               int* flag, void* stream) {
  DrawArgs p{};
  p.pic = picture; p.boxes = boxes; p.offsets = box_offsets; p.captions = captions; p.box_palette = box_palette;
  p.blob = blob; p.recs = records; p.flag = flag; p.blob_bytes = blob_bytes; p.tab = geom; p.size_tab = size_index;
  p.B = B; p.ih = ihm; p.iw = iwm; p.n_rows = n_rows; p.n_box_colors = n_box_colors; p.n_sizes = n_sizes;
  if (const int rc = captions_check("render_captions_ragged", p)) return rc;
  VR_CHECK_ARG(geom && size_index, "render_captions_ragged: needs the geometry table and the size-index table");
  return captions_launch<true>("render_captions_ragged", p, stream);
}
