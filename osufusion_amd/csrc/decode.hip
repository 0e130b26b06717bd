// The way back from a sampled signal to hit objects (osufusion_amd/decode.py is the host yardstick; osufusion_amd/decode_gpu.py calls these):
//
// osuf_decode_objects: (B, 6, L) fp32 samples -> the per-sample object table that decode_beatmap builds in its first forty lines, one
//   workgroup of 1024 lanes per sample, one launch per batch.  The four hit channels are discretised by sign into bit masks in LDS (64
//   frames per word, 4 x 1026 words = 32 KiB); every lane then owns one word: np.gradient + find_peaks of a +-1 row reduce to word
//   operations on the row shifted by -1, +1 and +2 frames, the object order comes from a popcount prefix sum over the workgroup, and
//   the lane that owns an onset looks up its run ends by scanning the SUSTAIN / SLIDER masks for the next zero bit.  No float atomics, no
//   global atomics; the result does not depend on scheduling.
//
//   Why the word operations are the host's rule.  With s in {-1, +1}, g = np.gradient(s) is (s[i+1] - s[i-1]) / 2 in {-1, 0, 1} inside and
//   s[1] - s[0], s[n-1] - s[n-2] in {-2, 0, 2} at the ends.  Repeat the end samples once (s[-1] := s[0], s[n] := s[n-1]): then
//   "g[k] >= 1" is  s[k+1] > 0 and not s[k-1] > 0  at every k, the ends included, and "g[k] == 1" is the same at an inner k.
//   _peaks_above(g, 0.5) takes the middle (i + j) // 2 of a plateau i..j of equal values >= 0.5 whose two neighbours are lower, 1 <= i,
//   j <= n - 2.  Such a plateau has the value 1 (an end sample is no peak) and at most two frames (g[i] = g[i+1] = g[i+2] = 1 would need
//   s[i+1] both > 0 and not), so its middle is i:  onset at i  <=>  g[i] == 1, not g[i-1] >= 1, and, if g[i+1] == 1, not g[i+2] >= 1,
//   else not g[i+1] >= 1.  The falling flips are the same rule on the complemented row.
//
// osuf_tempo_scan: for every (sample, candidate beat length) the fullest of the 100 phase bins of the onset times modulo the beat length
//   and the index of the first such bin -- np.histogram(t % bl, bins=100, range=(0, bl)) followed by max / argmax.  One wave per
//   candidate, integer LDS atomics (order-independent), fp64 throughout with contraction off.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kDecThreads = 1024;                     // one lane per 64-frame word: L <= 65 536
constexpr int kDecMaxL = 65536;
constexpr int kDecWords = kDecMaxL / 64;
constexpr int kDecRowWords = kDecWords + 2;           // word 0: frame 0 repeated (frames -64 .. -1); word nw + 1: frame n - 1 repeated
constexpr int kDecWaves = kDecThreads / 64;
constexpr int HIT_ROW = 0, SUSTAIN_ROW = 1, COMBO_ROW = 3;          // rows of the signal (SLIDER = SUSTAIN_ROW + 1)

typedef unsigned long long u64;

// bit i of the result = bit i + 1 / i + 2 / i - 1 of the stream (prev, cur, next)
__device__ inline u64 ahead1(u64 cur, u64 next) { return (cur >> 1) | (next << 63); }
__device__ inline u64 ahead2(u64 cur, u64 next) { return (cur >> 2) | (next << 62); }
__device__ inline u64 ahead3(u64 cur, u64 next) { return (cur >> 3) | (next << 61); }
__device__ inline u64 behind1(u64 prev, u64 cur) { return (cur << 1) | (prev >> 63); }
__device__ inline u64 behind2(u64 prev, u64 cur) { return (cur << 2) | (prev >> 62); }

// frames of this word at which the +-1 row flips (decode_flips); inner / inner_next = the frames 1 .. n - 2 of this word / the next one
__device__ inline u64 flips_word(u64 prev, u64 cur, u64 next, u64 inner, u64 inner_next) {
  u64 out = 0;
#pragma unroll
  for (int pol = 0; pol < 2; ++pol) {
    const u64 p = pol ? ~prev : prev, c = pol ? ~cur : cur, n = pol ? ~next : next;
    const u64 ge_m1 = c & ~behind2(p, c);                              // g[i-1] >= 1: s[i] and not s[i-2]
    const u64 ge_0 = ahead1(c, n) & ~behind1(p, c);                    // g[i]   >= 1
    const u64 ge_p1 = ahead2(c, n) & ~c;                               // g[i+1] >= 1
    const u64 ge_p2 = ahead3(c, n) & ~ahead1(c, n);                    // g[i+2] >= 1
    const u64 eq_p1 = ge_p1 & ahead1(inner, inner_next);               // g[i+1] == 1: >= 1 at an inner frame (an end frame holds 0, +-2)
    out |= ge_0 & inner & ~ge_m1 & ((eq_p1 & ~ge_p2) | (~eq_p1 & ~ge_p1));
  }
  return out;
}

// the frames 1 .. n - 2 among f0 .. f0 + 63
__device__ inline u64 inner_frames(int f0, int n) {
  const int last = n - 2 - f0;                                         // bit of frame n - 2
  if (last < 0) return 0;
  u64 m = last < 63 ? (~0ull >> (63 - last)) : ~0ull;
  if (f0 == 0) m &= ~1ull;
  return m;
}

// first frame z in [from, n) whose bit in `row` is clear, or -1
__device__ inline int next_clear(const u64* row, int from, int n, int nw) {
  int w = from >> 6;
  u64 word = ~row[w + 1] & (~0ull << (from & 63));
  while (word == 0 && ++w < nw) word = ~row[w + 1];
  if (word == 0) return -1;
  const int z = w * 64 + __builtin_ctzll(word);
  return z < n ? z : -1;
}

__global__ __launch_bounds__(kDecThreads) void decode_objects_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, int L, int cap, int* __restrict__ count, int* __restrict__ frame,
    int* __restrict__ sustain_end, int* __restrict__ slider_end, int* __restrict__ new_combo, double* __restrict__ px,
    double* __restrict__ py) {
  __shared__ u64 mask[4][kDecRowWords];
  __shared__ int wave_sum[kDecWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lengths ? lengths[b] : L;
  if (n < 2 || n > L) {                                                // uniform over the workgroup
    if (tid == 0) count[b] = 0;
    return;
  }
  const int nw = (n + 63) >> 6;
  const float* xb = x + (long)b * 6 * L;

  // the sign masks; a word's frames past n - 1 repeat frame n - 1
  for (int w = wave; w < nw; w += kDecWaves) {
    const int f = min(w * 64 + lane, n - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const u64 bits = __ballot(xb[(long)r * L + f] > 0.0f);             // 0.0, -0.0 and NaN: not positive
      if (lane == 0) mask[r][w + 1] = bits;
    }
  }
  __syncthreads();
  if (tid < 4) {
    mask[tid][0] = (mask[tid][1] & 1) ? ~0ull : 0ull;
    mask[tid][nw + 1] = (mask[tid][nw] >> 63) ? ~0ull : 0ull;           // bit 63 of the last word is frame n - 1 or its repeat
  }
  __syncthreads();

  // this lane's word of onsets and of combo flips
  u64 onsets = 0, combos = 0;
  if (tid < nw) {
    const u64 inner = inner_frames(tid * 64, n), inner_next = inner_frames(tid * 64 + 64, n);
    onsets = flips_word(mask[HIT_ROW][tid], mask[HIT_ROW][tid + 1], mask[HIT_ROW][tid + 2], inner, inner_next);
    combos = flips_word(mask[COMBO_ROW][tid], mask[COMBO_ROW][tid + 1], mask[COMBO_ROW][tid + 2], inner, inner_next);
  }
  const int stray = __syncthreads_or((combos & ~onsets) != 0);          // a combo flip at a frame that is no onset: marks the last object

  // exclusive prefix sum of the popcounts over the workgroup: the objects' order
  const int mine = __popcll(onsets);
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  int base = incl - mine, total = 0;
#pragma unroll
  for (int k = 0; k < kDecWaves; ++k) {
    const int s = wave_sum[k];
    if (k < wave) base += s;
    total += s;
  }
  if (tid == 0) count[b] = total;                                        // the true count, also past cap

  const long row = (long)b * cap;
  int k = base;
  while (onsets && k < cap) {
    const int bit = __builtin_ctzll(onsets);
    onsets &= onsets - 1;
    const int f = tid * 64 + bit;                                        // 1 <= f <= n - 2
    int ends[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {                                        // a run that starts exactly here: f not positive, f + 1 positive
      const u64* m = mask[SUSTAIN_ROW + r];
      const bool here = !((m[(f >> 6) + 1] >> (f & 63)) & 1), after = (m[((f + 1) >> 6) + 1] >> ((f + 1) & 63)) & 1;
      int e = -1;
      if (here && after) {
        const int z = next_clear(m, f + 1, n, nw);                       // no clear bit before n: the run is open at the end, no end
        if (z > 0) e = z - 1;
      }
      ends[r] = e;
    }
    frame[row + k] = f;
    sustain_end[row + k] = ends[0];
    slider_end[row + k] = ends[1];
    new_combo[row + k] = (int)((combos >> bit) & 1) | (stray && k == total - 1);
    px[row + k] = rint(((double)xb[4L * L + f] + 1.0) / 2.0 * 512.0);
    py[row + k] = rint(((double)xb[5L * L + f] + 1.0) / 2.0 * 384.0);
    ++k;
  }
}

constexpr int kScanThreads = 256, kScanWaves = kScanThreads / 64, kBins = 100;

__global__ __launch_bounds__(kScanThreads) void tempo_scan_kernel(
    const int* __restrict__ frame, const int* __restrict__ count, int cap, const double* __restrict__ frame_times, int L,
    const double* __restrict__ beat_len, int C, int* __restrict__ best_count, int* __restrict__ best_bin) {
  __shared__ int hist[kScanWaves][128];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * kScanWaves + wave;
  const bool live = c < C;
  hist[wave][lane] = 0;
  hist[wave][lane + 64] = 0;
  __syncthreads();
  if (live) {
    const double bl = beat_len[(long)b * C + c];
    const double width = bl / 100.0;
    const int n = min(max(count[b], 0), cap);
    const int* fr = frame + (long)b * cap;
    for (int i = lane; i < n; i += 64) {
      const int f = fr[i];
      if (f < 0 || f >= L) continue;
      const double t = frame_times[f];
      double ph = fmod(t, bl);                                           // np.remainder
      if (ph != 0.0) { if ((bl < 0.0) != (ph < 0.0)) ph += bl; }
      else ph = copysign(0.0, bl);
      if (!(ph >= 0.0 && ph <= bl)) continue;                            // outside the range (NaN included): not counted
      int idx = (int)(ph / bl * 100.0);                                  // numpy's uniform bins (_histograms_impl.py)
      if (idx == kBins) idx = kBins - 1;
      if (ph < (double)idx * width) --idx;
      const double upper = idx + 1 == kBins ? bl : (double)(idx + 1) * width;
      if (ph >= upper && idx != kBins - 1) ++idx;
      if (idx >= 0 && idx < kBins) atomicAdd(&hist[wave][idx], 1);
    }
  }
  __syncthreads();
  // the fullest bin, the first one on ties: max of count * 128 + (127 - bin)
  const int h0 = hist[wave][lane], h1 = lane + 64 < kBins ? hist[wave][lane + 64] : -1;
  int key = h0 * 128 + (127 - lane);
  if (h1 >= 0) key = max(key, h1 * 128 + (127 - (lane + 64)));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o, 64));
  if (live && lane == 0) {
    best_count[(long)b * C + c] = key >> 7;
    best_bin[(long)b * C + c] = 127 - (key & 127);
  }
}

}  // namespace

extern "C" int osuf_decode_objects(const float* x, const int* lengths, int B, int L, int cap, int* count, int* frame, int* sustain_end,
                                   int* slider_end, int* new_combo, double* px, double* py, hipStream_t stream) {
  if (!x || !count || !frame || !sustain_end || !slider_end || !new_combo || !px || !py) return OSUF_EINVAL;
  if (B < 1 || L < 2 || L > kDecMaxL || cap < 1) return OSUF_EINVAL;
  decode_objects_kernel<<<(unsigned)B, kDecThreads, 0, stream>>>(x, lengths, L, cap, count, frame, sustain_end, slider_end, new_combo, px, py);
  return osuf_launch_status();
}

extern "C" int osuf_tempo_scan(const int* frame, const int* count, int cap, const double* frame_times, int L, const double* beat_len,
                               int B, int C, int* best_count, int* best_bin, hipStream_t stream) {
  if (!frame || !count || !frame_times || !beat_len || !best_count || !best_bin) return OSUF_EINVAL;
  if (B < 1 || B > 65535 || C < 1 || L < 1 || cap < 1) return OSUF_EINVAL;
  const dim3 grid((unsigned)((C + kScanWaves - 1) / kScanWaves), (unsigned)B);
  tempo_scan_kernel<<<grid, kScanThreads, 0, stream>>>(frame, count, cap, frame_times, L, beat_len, C, best_count, best_bin);
  return osuf_launch_status();
}
