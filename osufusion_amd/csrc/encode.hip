// osuf_encode_signals: hit objects -> the six training signals (HIT, SUSTAIN, SLIDER, COMBO, CURSOR_X, CURSOR_Y), one thread per
// (sample, frame), one launch per batch.  Replaces the per-frame Python loops of the reference's library/osu/data/hit.py, cursor.py
// and encode.py.  Every frame is independent: no atomics, no LDS, no cross-lane traffic; the tables are read through binary searches.
//
// All comparisons and geometry run in fp64 in the order the fp64 yardstick (tests/encode_oracle.py) runs them, with contraction off, so
// that the selects (which object, which interval, which Bezier segment, which side of a half-integer) agree with it; the one rounding to
// fp32 happens after `* 2 - 1`.  Throughput of this kernel does not matter (a song is ~22 500 frames); agreement does.
//
// Tables (built by osufusion_amd/encode.py BeatmapTable; all indices are global, i.e. already offset per map):
//   map_hdr  int    [n_maps][8]   {n_obj, obj_off, n_sus, sus_off, n_sld, sld_off, 0, 0}
//   obj_f    double [objects][16] {t, end_time, start_x, start_y, end_x, end_y (rounded), start_x, start_y, end_x, end_y (unrounded),
//                                  slide_duration, g0, g1, g2, g3, g4}
//                                 Line: g = {ax, ay, bx, by, -}; Perfect: g = {cx, cy, r, theta0, theta1}; others unused.
//   obj_i    int    [objects][4]  {kind (0 circle, 1 spinner, 2 line, 3 perfect, 4 bezier), number of new-combo objects of the map up to
//                                  and including this one, seg_off, n_seg}
//   ivl      double [intervals][2] disjoint, sorted [s, e) per list: a map's SUSTAIN list at sus_off, its SLIDER list at sld_off
//   seg_cum  double [segments]    cum_t of a Bezier slider's segments (ascending, the last one 1.0)
//   seg_i    int    [segments][2] {node_off, degree}
//   nodes    double [nodes][2]    control points
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kEncThreads = 256;
constexpr int kObjF = 16, kObjI = 4;

// number of entries e of v[0 .. n) (stride `st` doubles) with e <= x
__device__ inline int count_le(const double* __restrict__ v, int n, int st, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[(long)mid * st] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// number of entries e of v[0 .. n) with e < x (numpy searchsorted from the left)
__device__ inline int count_lt(const double* __restrict__ v, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ inline double in_intervals(const double* __restrict__ ivl, int n, double t) {
  const int k = count_le(ivl, n, 2, t);                       // intervals that start at or before t; they are disjoint: test the last
  return (k > 0 && t < ivl[2L * (k - 1) + 1]) ? 1.0 : 0.0;
}

// position at the fraction ts of one slide
__device__ inline void slider_point(const double* __restrict__ of, const int* __restrict__ oi, const double* __restrict__ seg_cum,
                                    const int* __restrict__ seg_i, const double* __restrict__ nodes, double ts, double& px, double& py) {
  const int kind = oi[0];
  const double* g = of + 11;
  if (kind == 2) {
    px = (1.0 - ts) * g[0] + ts * g[2];
    py = (1.0 - ts) * g[1] + ts * g[3];
  } else if (kind == 3) {
    const double theta = (1.0 - ts) * g[3] + ts * g[4];
    px = g[0] + g[2] * cos(theta);
    py = g[1] + g[2] * sin(theta);
  } else {
    const int so = oi[2], ns = oi[3];
    const double* cum = seg_cum + so;
    const double u = fmin(1.0, fmax(0.0, ts));
    int idx = count_lt(cum, ns, u);
    if (idx >= ns) idx = ns - 1;                               // cum[ns - 1] == 1 >= u: never taken on a well-formed table
    const double lo = idx > 0 ? cum[idx - 1] : 0.0;
    const double s = (ts - lo) / (cum[idx] - lo);
    const int deg = seg_i[2L * (so + idx) + 1];
    const double* nd = nodes + 2L * seg_i[2L * (so + idx)];
    const double l1 = 1.0 - s, l2 = s;
    double rx = nd[0] * l1, ry = nd[1] * l1, pw = 1.0, binom = 1.0;
    for (int i = 1; i < deg; ++i) {                            // streaming Bernstein recurrence (beatmap.bezier_point)
      pw = pw * l2;
      binom = (binom * (double)(deg - i + 1)) / (double)i;
      const double w = binom * pw;
      rx = (rx + w * nd[2 * i]) * l1;
      ry = (ry + w * nd[2 * i + 1]) * l1;
    }
    const double w = l2 * pw;
    px = rx + w * nd[2 * deg];
    py = ry + w * nd[2 * deg + 1];
  }
}

__global__ __launch_bounds__(kEncThreads) void encode_kernel(
    const int* __restrict__ map_hdr, int n_maps, const double* __restrict__ obj_f, const int* __restrict__ obj_i,
    const double* __restrict__ ivl, const double* __restrict__ seg_cum, const int* __restrict__ seg_i, const double* __restrict__ nodes,
    const int* __restrict__ map_idx, const long* __restrict__ start, const int* __restrict__ len, const int* __restrict__ flip,
    int round_pos, float* __restrict__ out, double* __restrict__ pos_px, int L) {
  const int l = blockIdx.x * kEncThreads + threadIdx.x;
  const int b = blockIdx.y;
  if (l >= L) return;
  float* o = out + (long)b * 6 * L + l;
  const int m = map_idx[b];
  if (l >= len[b] || m < 0 || m >= n_maps) {                   // padding (data.collate_fn's -1.0); a map index outside the table: all padding
    for (int c = 0; c < 6; ++c) o[(long)c * L] = -1.0f;
    if (pos_px) { pos_px[((long)b * 2) * L + l] = 0.0; pos_px[((long)b * 2 + 1) * L + l] = 0.0; }
    return;
  }
  const int* h = map_hdr + 8L * m;
  const int n_obj = h[0];
  const double* of0 = obj_f + (long)h[1] * kObjF;
  const int* oi0 = obj_i + (long)h[1] * kObjI;
  const double t = (double)(start[b] + l) * 176.0 / 22050.0 * 1000.0;

  const int cnt = count_le(of0, n_obj, kObjF, t);              // objects with t_obj <= t: the current one is cnt - 1, the next one cnt
  const double hit = (double)(cnt & 1);
  const double combo = cnt > 0 ? (double)(oi0[(long)(cnt - 1) * kObjI + 1] & 1) : 0.0;
  const double sustain = in_intervals(ivl + 2L * h[3], h[2], t);
  const double slider = in_intervals(ivl + 2L * h[5], h[4], t);

  const int ps = round_pos ? 2 : 6;                            // start_pos / end_pos columns: rounded or not
  double px, py;
  if (n_obj <= 0) {
    px = 256.0; py = 192.0;
  } else if (cnt == 0) {
    px = of0[ps]; py = of0[ps + 1];
  } else {
    const double* of = of0 + (long)(cnt - 1) * kObjF;
    const int* oi = oi0 + (long)(cnt - 1) * kObjI;
    const double end = of[1];
    if (t < end) {
      if (oi[0] < 2) {                                         // a spinner (a circle ends where it starts and never gets here)
        px = of[ps]; py = of[ps + 1];
      } else {
        const double d = of[10];
        const double ts = fmod(t - of[0], d * 2.0) / d;
        slider_point(of, oi, seg_cum, seg_i, nodes, ts < 1.0 ? ts : 2.0 - ts, px, py);
        if (round_pos) { px = rint(px); py = rint(py); }
      }
    } else if (cnt == n_obj) {
      px = of[ps + 2]; py = of[ps + 3];
    } else {
      const double* nf = of + kObjF;
      const double f = (t - end) / (nf[0] - end);
      px = (1.0 - f) * of[ps + 2] + f * nf[ps];
      py = (1.0 - f) * of[ps + 3] + f * nf[ps + 1];
    }
  }
  if (pos_px) { pos_px[((long)b * 2) * L + l] = px; pos_px[((long)b * 2 + 1) * L + l] = py; }
  float cx = (float)(px / 512.0 * 2.0 - 1.0);
  float cy = (float)(py / 384.0 * 2.0 - 1.0);
  const int fl = flip ? flip[b] : 0;
  if (fl & 1) cx = __uint_as_float(__float_as_uint(cx) ^ 0x80000000u);     // the sign of the stored value: -0.0 where it was +0.0
  if (fl & 2) cy = __uint_as_float(__float_as_uint(cy) ^ 0x80000000u);
  o[0] = (float)(hit * 2.0 - 1.0);
  o[(long)L] = (float)(sustain * 2.0 - 1.0);
  o[2L * L] = (float)(slider * 2.0 - 1.0);
  o[3L * L] = (float)(combo * 2.0 - 1.0);
  o[4L * L] = cx;
  o[5L * L] = cy;
}

}  // namespace

extern "C" int osuf_encode_signals(const int* map_hdr, int n_maps, const double* obj_f, const int* obj_i, const double* ivl,
                                   const double* seg_cum, const int* seg_i, const double* nodes, const int* map_idx, const long* start,
                                   const int* len, const int* flip, int round_pos, float* out, double* pos_px, int B, int L, hipStream_t stream) {
  if (!map_hdr || !obj_f || !obj_i || !ivl || !seg_cum || !seg_i || !nodes || !map_idx || !start || !len || !out) return OSUF_EINVAL;
  if (n_maps <= 0 || B <= 0 || L <= 0 || B > 65535) return OSUF_EINVAL;
  const dim3 grid((unsigned)((L + kEncThreads - 1) / kEncThreads), (unsigned)B);
  encode_kernel<<<grid, kEncThreads, 0, stream>>>(map_hdr, n_maps, obj_f, obj_i, ivl, seg_cum, seg_i, nodes, map_idx, start, len, flip,
                                                 round_pos, out, pos_px, L);
  return osuf_launch_status();
}
