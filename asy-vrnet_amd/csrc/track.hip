// Multi-object tracking of the kept detections, on the device: every batch slot is a STREAM of successive frames of one
// camera, and a fixed-capacity table of tracks per stream lives in device memory across calls (and across replays of a
// captured graph).  One launch per call predicts every track, matches tracks and detection rows greedily by IoU, filters
// the matched tracks (box and, with the radar readout of csrc/boxradar.hip, range), coasts and frees the others, starts new
// tracks and writes a track id per detection row.  The reference has no tracker; the rule is this project's definition,
// stated on the host by data.track_update, which this kernel equals bit for bit (float32, one rounding per operation,
// contraction off; the quotient of the IoU is the correctly rounded division).
//
// One workgroup of 256 per stream.  Thread s owns slot s of the table (T <= 256) in registers; the boxes of the live slots
// and of the valid rows (cap <= 1024) lie in LDS, about 43 KB.  The greedy matching is done in its mutually-best form: in a
// round wave w takes the unmatched live slots w, w + 4, ..., its lanes sweep the unmatched valid rows of the slot's class and
// compute the 64-bit key bits(iou) << 32 | (65535 - slot) << 16 | (65535 - row) of every candidate pair (iou >= thr).  The
// largest key of a slot comes from a wave reduction (shuffles) into the slot's LDS word, the largest key of a row from an
// integer LDS atomic maximum.  A pair whose key is the largest of its slot AND of its row is matched; keys are unique, so
// that is exactly the set of pairs the one-at-a-time greedy loop would take among them, and the rounds repeat until one
// matches nothing.  The IoU matrix is never stored: a round recomputes what it needs, and later rounds skip matched slots
// and rows.  Births: two exclusive block scans, one over the valid unmatched rows and one over the free slots, pair the k-th
// such row with the k-th free slot.  Integer atomics only (LDS; the one global atomic is the OR into *flag); every word of
// table, head and ids is a pure function of the inputs: the same bytes on every run.
#include "common.h"
#include "wgscan.h"

#pragma clang fp contract(off)

extern "C" {
/* include/vrnet_hip.h: one track (64 bytes); data.TRACK_DTYPE mirrors it.  A free slot is all zeros. */
typedef struct vrnet_track {
  int id, cls, hits, misses, row, range_age;
  float x[5], v[5];
} vrnet_track;
}
static_assert(sizeof(vrnet_track) == 64 && alignof(vrnet_track) == 4 && offsetof(vrnet_track, x) == 24 &&
                  offsetof(vrnet_track, v) == 44,
              "vrnet_track is 16 words: data.TRACK_DTYPE mirrors it");

namespace {

constexpr int TK_THREADS = 256, TK_WAVES = 4;
static_assert(TK_THREADS == VR_WG_THREADS && TK_WAVES == VR_WG_WAVES, "tk_scan is the 256-thread scan of wgscan.h over part[TK_WAVES]");
constexpr int TK_MAX_TRACKS = 256, TK_MAX_ROWS = 1024;
constexpr int TK_ROW_FLOATS = 7;     // top, left, bottom, right, obj, class_conf, class
constexpr int TK_HEAD = 4;           // ids handed out, live tracks, calls, births of this call
constexpr int TK_INT_MAX = 2147483647;

struct TrackArgs {
  const float* rows;                 // (B, cap, 7)
  const int* kept;                   // (B)
  int B, cap, T;
  vrnet_track* table;                // (B, T)
  int* head;                         // (B, 4)
  int* ids;                          // (B, cap)
  const int* box_points;             // (B, cap) or null
  const float* box_radar;            // (B, cap, 2, 5) or null
  float thr;
  int max_age;
  float g_pos, g_vel, rg_pos, rg_vel;
  int* flag;                         // or null
};

__device__ __forceinline__ bool tk_finite(float a) { return fabsf(a) < INFINITY; }

// data.track_iou of one pair
__device__ __forceinline__ float tk_iou(float t1, float l1, float b1, float r1, float t2, float l2, float b2, float r2) {
  const float ih = (b1 < b2 ? b1 : b2) - (t1 > t2 ? t1 : t2);
  const float iw = (r1 < r2 ? r1 : r2) - (l1 > l2 ? l1 : l2);
  if (!(ih > 0.f && iw > 0.f)) return 0.f;
  const float inter = ih * iw;
  const float a1 = (b1 - t1) * (r1 - l1), a2 = (b2 - t2) * (r2 - l2);
  const float uni = (a1 + a2) - inter;
  return inter / uni;
}

// exclusive scan of one 0 / 1 value per thread over the 256 threads; tot: the sum.  part: four slots; ends behind a barrier
__device__ __forceinline__ int tk_scan(int own, int* part, int& tot) {
  __syncthreads();                     // the slots may still be read from the scan before
  return vr_block_scan_incl<vr_op_sum>(own, part, tot) - own;
}

// step 3's range update of one record from row i of the readout
__device__ __forceinline__ void tk_range(const TrackArgs& p, long row, vrnet_track& r) {
  if (!p.box_points || !(p.box_points[row] > 0)) return;
  const float depth = p.box_radar[row * 10 + 5];          // the lower median's depth
  if (!tk_finite(depth)) return;
  if (r.range_age < 0) {
    r.x[4] = depth;
    r.v[4] = 0.f;
  } else {
    const float d = depth - r.x[4];
    r.x[4] = r.x[4] + p.rg_pos * d;
    r.v[4] = r.v[4] + p.rg_vel * d;
  }
  r.range_age = 0;
}

__global__ __launch_bounds__(TK_THREADS) void track_update_kernel(const TrackArgs p) {
  __shared__ float zt[TK_MAX_ROWS], zl[TK_MAX_ROWS], zb[TK_MAX_ROWS], zr[TK_MAX_ROWS];
  __shared__ int zcls[TK_MAX_ROWS];
  __shared__ int row_slot[TK_MAX_ROWS];                   // -2: not valid, -1: valid and unmatched, else the slot
  __shared__ unsigned long long row_best[TK_MAX_ROWS];
  __shared__ float xt[TK_MAX_TRACKS], xl[TK_MAX_TRACKS], xb[TK_MAX_TRACKS], xr[TK_MAX_TRACKS];
  __shared__ int xcls[TK_MAX_TRACKS];
  __shared__ int slot_row[TK_MAX_TRACKS];                 // -2: not live, -1: live and unmatched, else the row
  __shared__ unsigned long long slot_best[TK_MAX_TRACKS];
  __shared__ int free_slot[TK_MAX_TRACKS];                // the k-th free slot
  __shared__ int part[TK_WAVES];
  __shared__ int matched[2];                              // pairs matched in a round, double-buffered by round parity
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = p.T, cap = p.cap;
  const int raw_kept = p.kept[b];
  const int n = vr_clampi(raw_kept, 0, cap);
  int bits = n != raw_kept ? VR_FLAG_BOX_COUNT : 0;
  const float* rows = p.rows + (long)b * cap * TK_ROW_FLOATS;
  vrnet_track* table = p.table + (long)b * T;
  const int next_id = p.head[b * TK_HEAD];                // read in front of the barriers: thread 0 writes it at the end

  // the rows of this call
  for (int i = tid; i < n; i += TK_THREADS) {
    const float* q = rows + (long)i * TK_ROW_FLOATS;
    const float t = q[0], l = q[1], bo = q[2], r = q[3], c = q[6];
    const bool valid = tk_finite(t) && tk_finite(l) && tk_finite(bo) && tk_finite(r) && bo > t && r > l;
    zt[i] = t;  zl[i] = l;  zb[i] = bo;  zr[i] = r;
    zcls[i] = (c >= -2147483648.f && c < 2147483648.f) ? (int)c : -1;
    row_slot[i] = valid ? -1 : -2;
  }
  // 1 predict: thread s owns slot s
  vrnet_track rec{};
  bool live = false;
  if (tid < T) {
    rec = table[tid];
    live = rec.id != 0;
    if (live) {
#pragma unroll
      for (int k = 0; k < 4; ++k) rec.x[k] = rec.x[k] + rec.v[k];
      if (rec.range_age >= 0) {
        rec.x[4] = rec.x[4] + rec.v[4];
        if (rec.range_age < TK_INT_MAX) ++rec.range_age;
      }
      if (!(tk_finite(rec.x[0]) && tk_finite(rec.x[1]) && tk_finite(rec.x[2]) && tk_finite(rec.x[3]))) {
        rec = vrnet_track{};
        live = false;
      }
    }
    xt[tid] = rec.x[0];  xl[tid] = rec.x[1];  xb[tid] = rec.x[2];  xr[tid] = rec.x[3];
    xcls[tid] = rec.cls;
    slot_row[tid] = live ? -1 : -2;
  }
  if (tid < 2) matched[tid] = 0;
  __syncthreads();

  // 2 match: rounds of mutually-best pairs
  for (int round = 0;; ++round) {
    for (int i = tid; i < n; i += TK_THREADS) row_best[i] = 0ULL;
    __syncthreads();
    if (tid == 0) matched[(round + 1) & 1] = 0;            // the next round's counter: every thread has read it by now
    for (int s = wave; s < T; s += TK_WAVES) {            // wave-uniform
      if (slot_row[s] != -1) continue;
      const float t1 = xt[s], l1 = xl[s], b1 = xb[s], r1 = xr[s];
      const int c1 = xcls[s];
      unsigned long long best = 0ULL;
      for (int i = lane; i < n; i += 64) {
        if (row_slot[i] != -1 || zcls[i] != c1) continue;
        const float iou = tk_iou(t1, l1, b1, r1, zt[i], zl[i], zb[i], zr[i]);
        if (!(iou >= p.thr)) continue;                    // a NaN is no candidate
        const unsigned long long key = ((unsigned long long)__float_as_uint(iou) << 32) | ((unsigned)(65535 - s) << 16) |
                                       (unsigned)(65535 - i);
        atomicMax(&row_best[i], key);
        best = key > best ? key : best;
      }
      if (__any(best != 0ULL)) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long other = vr_shfl_xor64(best, o);
          best = other > best ? other : best;
        }
      }
      if (lane == 0) slot_best[s] = best;                 // this wave alone owns slot s
    }
    __syncthreads();
    if (tid < T && slot_row[tid] == -1) {
      const unsigned long long key = slot_best[tid];
      if (key != 0ULL) {
        const int i = 65535 - (int)(key & 0xFFFFu);
        if (row_best[i] == key) {                         // the best of its row too: unique keys, so one slot per row
          slot_row[tid] = i;
          row_slot[i] = tid;
          atomicAdd(&matched[round & 1], 1);
        }
      }
    }
    __syncthreads();
    if (matched[round & 1] == 0) break;                   // uniform: read behind the barrier, cleared two rounds later
  }

  // 3 update, 4 coast
  if (live) {
    const int i = slot_row[tid];
    if (i >= 0) {
      const float z[4] = {zt[i], zl[i], zb[i], zr[i]};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = z[k] - rec.x[k];
        rec.x[k] = rec.x[k] + p.g_pos * d;
        rec.v[k] = rec.v[k] + p.g_vel * d;
      }
      if (rec.hits < TK_INT_MAX) ++rec.hits;
      rec.misses = 0;
      rec.row = i;
      tk_range(p, (long)b * cap + i, rec);
    } else {
      ++rec.misses;
      rec.row = -1;
      if (rec.misses > p.max_age) {
        rec = vrnet_track{};
        live = false;
      }
    }
  }

  // 5 births: the k-th valid unmatched row takes the k-th free slot
  const bool is_free = tid < T && !live;
  int n_free;
  const int free_rank = tk_scan(is_free ? 1 : 0, part, n_free);
  if (is_free) free_slot[free_rank] = tid;
  // rows: thread t scans the rows [t * per, t * per + per)
  const int per = (n + TK_THREADS - 1) / TK_THREADS;       // at most 4
  const int first = tid * per;
  int own = 0;
  for (int i = first; i < first + per && i < n; ++i) own += row_slot[i] == -1 ? 1 : 0;
  // an exclusive scan of `own` (0..4): the 0 / 1 scan serves, bit by bit of the count
  int n_new = 0, new_rank = 0;
  {
    int t0, t1, t2;
    const int r0 = tk_scan(own & 1, part, t0), r1 = tk_scan((own >> 1) & 1, part, t1), r2 = tk_scan((own >> 2) & 1, part, t2);
    new_rank = r0 + 2 * r1 + 4 * r2;
    n_new = t0 + 2 * t1 + 4 * t2;
  }
  const int births = n_new < n_free ? n_new : n_free;      // free_slot is complete: tk_scan ended behind a barrier
  if (n_new > n_free) bits |= VR_FLAG_TRACK_FULL;
  int* ids = p.ids + (long)b * cap;
  {
    int k = new_rank;
    for (int i = first; i < first + per && i < n; ++i) {
      const int s = row_slot[i];
      int id = 0;
      if (s >= 0) {
        id = -1;                                          // the slot's thread writes it below
      } else if (s == -1) {
        if (k < births) {
          vrnet_track born{};
          born.id = id = next_id + k + 1;
          born.cls = zcls[i];
          born.hits = 1;
          born.row = i;
          born.range_age = -1;
          born.x[0] = zt[i];  born.x[1] = zl[i];  born.x[2] = zb[i];  born.x[3] = zr[i];
          tk_range(p, (long)b * cap + i, born);
          table[free_slot[k]] = born;
        }
        ++k;
      }
      if (id >= 0) ids[i] = id;
    }
  }
  for (int i = n + tid; i < cap; i += TK_THREADS) ids[i] = 0;
  if (tid < T) {
    if (live && rec.row >= 0) ids[rec.row] = rec.id;
    if (!(is_free && free_rank < births)) table[tid] = rec;   // a free slot that a row took is that row's to write
  }
  if (tid == 0) {
    int* head = p.head + b * TK_HEAD;
    head[0] = next_id + births;
    head[1] = T - n_free + births;
    head[2] = head[2] + 1;
    head[3] = births;
    if (bits && p.flag) atomicOr(p.flag, bits);
  }
}

}  // namespace

extern "C" int vrnet_track_update_f32(const float* rows, const int* kept, int B, int cap, vrnet_track* table, int max_tracks,
                                      int* head, int* ids_out, const int* box_points, const float* box_radar, float iou,
                                      int max_age, float gain_pos, float gain_vel, float range_gain_pos, float range_gain_vel,
                                      int* flag, void* stream) {
  const char* who = "track_update";
  VR_CHECK_ARG(rows && kept && table && head && ids_out, "%s: rows, kept, table, head and ids_out are required", who);
  VR_CHECK_ARG(B > 0 && B < 65536 && cap > 0 && cap <= TK_MAX_ROWS && max_tracks > 0 && max_tracks <= TK_MAX_TRACKS,
               "%s: bad shape (B %d, cap %d of at most %d, max_tracks %d of at most %d)", who, B, cap, TK_MAX_ROWS, max_tracks,
               TK_MAX_TRACKS);
  VR_CHECK_ARG((box_points == nullptr) == (box_radar == nullptr), "%s: box_points and box_radar come together or not at all", who);
  VR_CHECK_ARG(iou > 0.f && iou <= 1.f, "%s: iou must lie in (0, 1], got %g", who, (double)iou);
  VR_CHECK_ARG(max_age >= 0 && max_age <= (1 << 20), "%s: max_age must lie in [0, 2^20], got %d", who, max_age);
  const float gains[4] = {gain_pos, gain_vel, range_gain_pos, range_gain_vel};
  for (float g : gains) VR_CHECK_ARG(g >= 0.f && g <= 2.f, "%s: every gain must lie in [0, 2], got %g", who, (double)g);
  TrackArgs p{};
  p.rows = rows; p.kept = kept; p.B = B; p.cap = cap; p.T = max_tracks;
  p.table = table; p.head = head; p.ids = ids_out;
  p.box_points = box_points; p.box_radar = box_radar;
  p.thr = iou; p.max_age = max_age;
  p.g_pos = gain_pos; p.g_vel = gain_vel; p.rg_pos = range_gain_pos; p.rg_vel = range_gain_vel;
  p.flag = flag;
  hipLaunchKernelGGL(track_update_kernel, dim3((unsigned)B), dim3(TK_THREADS), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK(who);
  return VR_OK;
}
