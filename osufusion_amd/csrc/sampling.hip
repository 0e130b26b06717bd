// The sampling kernels (HBM-bound, fp32, 16 B per lane where the buffers allow), gfx950: the discrete DDPM / DDIM algebra, continuous-time
// Gaussian diffusion (log-SNR schedule, the step kernel of the ancestral sampler and of the DDIM / DPM-Solver++(2M) solvers, the dynamic
// threshold's radix select, q_sample), masked generation, the windows of windowed sampling and the rescale of the guided prediction; their
// entry points follow the kernels.
#include "common.hpp"

// ---- DDPM / DDIM algebra on (B, D, L) fp32 tensors; per-sample coefficients in device arrays -------------
// out = ca[b] * x + cb[b] * y                      add_noise: ca = sqrt(acp_t), cb = sqrt(1 - acp_t)
__global__ __launch_bounds__(256) void axpby_rows_kernel(const float* x, const float* y, const float* ca, const float* cb, float* out,
                                                         long per_sample, long total) {
  GRID_STRIDE(idx, total) {
    const long b = idx / per_sample;
    out[idx] = ca[b] * x[idx] + cb[b] * y[idx];
  }
}

// DDIM step (eta = 0, epsilon prediction, clip_sample): coef[b] = {sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev)}
// eps = null + (cond - null) * cond_scale when `null` is given (classifier-free guidance, unet.py:458-465)
__global__ __launch_bounds__(256) void ddim_step_kernel(const float* x, const float* cond, const float* nullp, float cond_scale,
                                                        const float* coef, float* out, long per_sample, long total) {
  GRID_STRIDE(idx, total) {
    const long b = idx / per_sample;
    float eps = cond[idx];
    if (nullp) { const float nu = nullp[idx]; eps = nu + (eps - nu) * cond_scale; }
    const float* c = coef + 4 * b;
    float x0 = (x[idx] - c[0] * eps) / c[1];
    x0 = fminf(fmaxf(x0, -1.f), 1.f);
    out[idx] = c[2] * x0 + c[3] * eps;
  }
}

// ---- continuous-time Gaussian diffusion (scheduler.py): log-SNR schedule and the ancestral (DDPM) step ----------------------------
// log_snr(t) in fp32, in the reference's order of operations (scheduler.py:11-23 as torch evaluates it on fp32 tensors: t**2 = t*t,
// x**-2 = 1/(x*x), python scalars rounded to fp32).  The network is conditioned on this fp32 value, and it is not the fp64 one: the
// cosine schedule cancels in cos(.)^-2 - 1 and takes cos of an fp32 argument at pi/2.  No contraction: 10*(t*t) + 1e-4 stays two roundings.
// Every intermediate is an fp32 value; the transcendental functions (ct_cos, ct_log, ...) are correctly rounded fp32 functions, the fp64
// routine rounded once.  A 1-ulp fp32 routine agrees with another libm's in most arguments only, and one ulp of log_snr = -33.9 is a
// relative 2e-6 of alpha; the correctly rounded result is what a careful libm returns (B values per launch: the cost is nothing).
#define CT_FN(name, fn) __device__ inline float name(float x) { return (float)fn((double)x); }
CT_FN(ct_cos, cos) CT_FN(ct_log, log) CT_FN(ct_exp, exp) CT_FN(ct_expm1, expm1)
#undef CT_FN

__device__ inline float ct_log_snr(float t, int kind) {
#pragma clang fp contract(off)
  if (kind == 0) {                                       // linear: -log(expm1(1e-4 + 10 t^2))
    const float u = 1e-4f + 10.f * (t * t);
    return -ct_log(ct_expm1(u));
  }
  const float a = (t + 0.008f) / 1.008f * 3.14159265358979323846f * 0.5f;      // cosine: -log(max(cos(.)^-2 - 1, 1e-8))
  const float c = ct_cos(a);
  const float r = 1.f / (c * c) - 1.f;
  return -ct_log(fmaxf(r, 1e-8f));
}

__device__ inline float ct_sigmoid(float x) { return 1.f / (1.f + ct_exp(-x)); }

// One thread per sample.  Row of `cols` floats (OSUF_CT_COLS_T = 3 without t_next, OSUF_CT_COLS = 13 with it):
//   0 log_snr  1 alpha  2 sigma | 3 log_snr_next  4 alpha_next  5 sigma_next  6 c = -expm1(log_snr - log_snr_next)
//   7 posterior_variance = sigma_next^2 c  8 posterior_log_variance = log(max(var, 1e-20))            (scheduler.py:83-93)
//   9 1 / max(alpha, 1e-8)  10 alpha_next (1 - c) / alpha  11 alpha_next c  12 noise gain = t_next > 0 ? exp(0.5 log_var) : 0
__global__ __launch_bounds__(256) void ct_schedule_kernel(const float* t, const float* t_next, int kind, float* out, int B) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float ls = ct_log_snr(t[b], kind);
  const float alpha = sqrtf(ct_sigmoid(ls)), sigma = sqrtf(ct_sigmoid(-ls));
  float* o = out + (long)b * (t_next ? 13 : 3);
  o[0] = ls; o[1] = alpha; o[2] = sigma;
  if (!t_next) return;
  const float tn = t_next[b];
  const float lsn = ct_log_snr(tn, kind);
  const float alpha_n = sqrtf(ct_sigmoid(lsn)), sigma_n = sqrtf(ct_sigmoid(-lsn));
  const float c = -ct_expm1(ls - lsn);
  const float var = (sigma_n * sigma_n) * c;
  const float logvar = ct_log(fmaxf(var, 1e-20f));
  o[3] = lsn; o[4] = alpha_n; o[5] = sigma_n; o[6] = c; o[7] = var; o[8] = logvar;
  o[9] = 1.f / fmaxf(alpha, 1e-8f);
  o[10] = alpha_n * ((1.f - c) / alpha);
  o[11] = alpha_n * c;
  o[12] = tn > 0.f ? ct_exp(0.5f * logvar) : 0.f;
}

// The ancestral step: eps = null + (cond - null) cond_scale;  x0 = clamp((x - sigma eps) / max(alpha, 1e-8), -1, 1);
// mean = alpha_next (x (1 - c) / alpha + c x0);  out = mean + gain * noise.  k = the sample's schedule row.  A zero gain (t_next == 0) or no
// noise buffer: the mean, whatever noise holds.  The kernel is ct_step_kernel below, which the solvers share.
// OBJ = what the network predicts (OSUF_CT_OBJ_*): the start prediction is (x - sigma p) / max(alpha, 1e-8) for noise, p itself for x_start and
// alpha x - sigma p for v.  THR: the sample's dynamic threshold s (>= 1, osuf_ct_x0_quantile) replaces the static clamp: clamp(x0, -s, s) / s.
template <int OBJ>
__device__ inline float ct_start(float x, float p, const float* k) {
  if (OBJ == 1) return p;
  if (OBJ == 2) return k[1] * x - k[2] * p;
  return (x - k[2] * p) * k[9];
}

// Classifier-free guidance: the prediction the step takes, from the conditional one and the null one.
__device__ inline float ct_guide(float cond, float nu, float cond_scale) { return nu + (cond - nu) * cond_scale; }

// The start prediction of the guided prediction p, clamped to [-1, 1] or (THR) to the sample's threshold and rescaled: what the ancestral step
// and the solver step (below) both take as x0.
template <int OBJ, bool THR>
__device__ inline float ct_start_clamped(float x, float p, const float* k, const float* s) {
  const float x0 = ct_start<OBJ>(x, p, k);
  if (THR) { const float sv = *s; return fminf(fmaxf(x0, -sv), sv) / sv; }
  return fminf(fmaxf(x0, -1.f), 1.f);
}

// ---- solvers on a log-SNR grid: DDIM(eta) and DPM-Solver++(2M) in data prediction -------------------------------------------------------
// Both are x_next = k_x x + k_0 x0 + k_p x0_prev + gain z, x0 the clamped start prediction (ct_start_clamped).  With lambda = log_snr / 2 and
// d = ls - ls_next (< 0 on a rising grid), c = -expm1(d), h = -d / 2:
//   DDIM(eta): sigma_eta = eta sqrt(sigma_n^2 / sigma^2 (1 - alpha^2 / alpha_n^2)) = eta sqrt(sigma_n^2 c)  (alpha^2 / sigma^2 = exp(ls): the
//     posterior variance), k_eps = sqrt(sigma_n^2 - sigma_eta^2) = sigma_n sqrt((1 - eta^2) + eta^2 exp(d)); k_x = k_eps / sigma,
//     k_0 = alpha_n - k_eps alpha / sigma with alpha / sigma = exp(ls / 2), gain = sigma_eta.  The right-hand forms are the ones evaluated:
//     sums of positive terms, where the left-hand ones cancel (1 - alpha^2 / alpha_n^2 at small h, sigma_n^2 - sigma_eta^2 at eta = 1 and
//     large h).  eta = 0: k_eps = sigma_n exactly.
//   DPM-Solver++(2M): k_d = -alpha_n expm1(-h), k_x = sigma_n / sigma; first step k_0 = k_d, k_p = 0 (= DDIM(0)); later steps, r = h_prev / h:
//     k_0 = k_d (1 + 1 / (2r)), k_p = -k_d / (2r).  gain = 0.
// One thread per step i of the grid ls[0 .. S] (rising; equal neighbours divide by zero in r): the step's 13-column row, written B times
// (rows[i][b][13], so that osuf_ct_x0_quantile and the step kernels index a step's rows by sample as they do osuf_ct_schedule's), and
// fac[i][4] = k_x, k_0, k_p, gain, one per step.  Row columns 0-11 by ct_schedule_kernel's expressions on (ls[i], ls[i + 1]); column 12, the
// ancestral gain, is zero on the last step (where ct_schedule_kernel has t_next = 0): a row is a valid osuf_ct_step_ex row too.
__global__ __launch_bounds__(256) void ct_solver_schedule_kernel(const float* ls_grid, int S, int sampler, float eta, float* rows, float* fac,
                                                                 int B) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  const float ls = ls_grid[i], lsn = ls_grid[i + 1];
  const float alpha = sqrtf(ct_sigmoid(ls)), sigma = sqrtf(ct_sigmoid(-ls));
  const float sig2_n = ct_sigmoid(-lsn);
  const float alpha_n = sqrtf(ct_sigmoid(lsn)), sigma_n = sqrtf(sig2_n);
  const float d = ls - lsn;
  const float c = -ct_expm1(d);
  const float var = (sigma_n * sigma_n) * c;
  const float logvar = ct_log(fmaxf(var, 1e-20f));
  const float row[13] = {ls, alpha, sigma, lsn, alpha_n, sigma_n, c, var, logvar, 1.f / fmaxf(alpha, 1e-8f), alpha_n * ((1.f - c) / alpha),
                         alpha_n * c, i < S - 1 ? ct_exp(0.5f * logvar) : 0.f};
  for (int b = 0; b < B; ++b) {
    float* o = rows + ((long)i * B + b) * 13;
    for (int j = 0; j < 13; ++j) o[j] = row[j];
  }
  float k_x, k_0, k_p = 0.f, gain = 0.f;
  if (sampler == OSUF_CT_SAMPLER_DDIM) {
    const float e2 = eta * eta;
    gain = eta * sqrtf(fmaxf(sig2_n * c, 0.f));
    const float exp_d = ct_exp(ls) * ct_exp(-lsn);         // not ct_exp(d): over a long step d's own rounding (2^-24 |d|) is the error of exp(d)
    const float k_eps = sigma_n * sqrtf((1.f - e2) + e2 * exp_d);
    k_x = k_eps / sigma;
    k_0 = alpha_n - k_eps * ct_exp(0.5f * ls);
  } else {
    const float h = 0.5f * (lsn - ls);
    const float k_d = -(alpha_n * ct_expm1(-h));
    k_x = sigma_n / sigma;
    k_0 = k_d;
    if (i > 0) {
      const float h_prev = 0.5f * (ls - ls_grid[i - 1]);
      const float q = (0.5f * h) / h_prev;                 // 1 / (2r)
      k_0 = k_d * (1.f + q);
      k_p = -(k_d * q);
    }
  }
  float* f = fac + 4 * (long)i;
  f[0] = k_x; f[1] = k_0; f[2] = k_p; f[3] = gain;
}

// ---- the step kernel: ancestral (osuf_ct_step_ex) and solver (osuf_ct_solver_step) ----------------------------------------------------------
// Both are x_next = k_x x + k_0 x0 (+ k_p x0_prev) (+ gain z), x0 the clamped start prediction of the guided prediction p.  SOLVER selects
// where the factors come from, whether x0_prev can enter, whether x0 is stored and how null, x0_prev and noise are read:
//   ancestral: columns 10, 11, -, 12 of the sample's row k (the posterior mean and its noise gain), no x0_prev, x_next alone is written; null
//     and noise are read element by element, noise only where the sample's gain is non-zero (t_next == 0: the mean, whatever the noise
//     buffer holds);
//   solver: f = the step's fac[0 .. 3], the same for every sample; x0 is written too, the next 2M step's x0_prev; the vector path reads the
//     three four at a time (its launch checks their alignment).
// One element.  LOADED: the caller has read nu, prev and z (the solver's vector path); otherwise null, x0_prev and noise are read here,
// element idx.  use_prev / use_noise: whether x0_prev and noise enter at all (the buffer is given and, for the solver, its factor is
// non-zero).
template <bool SOLVER, bool LOADED, int OBJ, bool THR>
__device__ inline float ct_step_one(float x, float cond, float nu, float prev, float z, const float* nullp, const float* x0_prev, const float* noise,
                                    long idx, float cond_scale, const float* k, const float* s, const float* f, bool use_prev, bool use_noise,
                                    float* x0_out) {
  const float p = nullp ? ct_guide(cond, LOADED ? nu : nullp[idx], cond_scale) : cond;
  if (SOLVER && !LOADED) {                                   // the solver reads ahead: both conditions are uniform over the launch
    prev = use_prev ? x0_prev[idx] : 0.f;
    z = use_noise ? noise[idx] : 0.f;
  }
  const float x0 = ct_start_clamped<OBJ, THR>(x, p, k, s);
  if (SOLVER) *x0_out = x0;
  float out = (SOLVER ? f[0] : k[10]) * x + (SOLVER ? f[1] : k[11]) * x0;
  if (SOLVER && use_prev) out += f[2] * prev;
  const float gain = SOLVER ? f[3] : k[12];
  if (use_noise && (SOLVER || gain != 0.f)) out += gain * (SOLVER ? z : noise[idx]);
  return out;
}

// VEC: four elements per lane over the flat (B * per_sample) range (a group may straddle two samples when per_sample is no multiple of 4: the
// row is looked up per element there) and a scalar tail of total % 4 elements; x, cond and x_next are 16-byte aligned, and for the solver
// every other buffer that is given.  s (THR only): sample b's threshold is s[b * s_ld], so that column 2 of osuf_ct_x0_quantile's rows is
// read in place.  fac, x0_prev and x0 are the solver's (null for the ancestral step, which does not touch them).
template <bool VEC, bool SOLVER, int OBJ, bool THR>
__global__ __launch_bounds__(256) void ct_step_kernel(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef,
                                                      const float* fac, const float* x0_prev, const float* noise, const float* s, long s_ld,
                                                      float* x_next, float* x0, long per_sample, long total) {
  float f[4] = {0.f, 0.f, 0.f, 0.f};
  if (SOLVER) { f[0] = fac[0]; f[1] = fac[1]; f[2] = fac[2]; f[3] = fac[3]; }
  const bool use_prev = SOLVER && x0_prev && f[2] != 0.f, use_noise = noise && (!SOLVER || f[3] != 0.f);
  auto scalar = [&](long idx) {
    const long b = idx / per_sample;
    x_next[idx] = ct_step_one<SOLVER, false, OBJ, THR>(x[idx], cond[idx], 0.f, 0.f, 0.f, nullp, x0_prev, noise, idx, cond_scale, coef + 13 * b,
                                                       THR ? s + b * s_ld : nullptr, f, use_prev, use_noise, SOLVER ? x0 + idx : nullptr);
  };
  if (!VEC) {
    GRID_STRIDE(idx, total) scalar(idx);
    return;
  }
  const long groups = total >> 2;
  GRID_STRIDE(g, groups) {
    const long i0 = g << 2;
    const long b0 = i0 / per_sample;
    const long left = (b0 + 1) * per_sample - i0;          // elements of this group's first sample from i0 on (>= 1)
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[g], cv = reinterpret_cast<const f32x4*>(cond)[g];
    f32x4 nv = {0.f, 0.f, 0.f, 0.f}, pv = nv, zv = nv, ov, sv;
    if (SOLVER && nullp) nv = reinterpret_cast<const f32x4*>(nullp)[g];
    if (use_prev) pv = reinterpret_cast<const f32x4*>(x0_prev)[g];
    if (SOLVER && use_noise) zv = reinterpret_cast<const f32x4*>(noise)[g];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long b = e < left ? b0 : (i0 + e) / per_sample;
      float x0e = 0.f;
      ov[e] = ct_step_one<SOLVER, SOLVER, OBJ, THR>(xv[e], cv[e], nv[e], pv[e], zv[e], nullp, x0_prev, noise, i0 + e, cond_scale, coef + 13 * b,
                                                    THR ? s + b * s_ld : nullptr, f, use_prev, use_noise, &x0e);
      sv[e] = x0e;
    }
    reinterpret_cast<f32x4*>(x_next)[g] = ov;
    if (SOLVER) reinterpret_cast<f32x4*>(x0)[g] = sv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (total & 3)) scalar((groups << 2) + threadIdx.x);
}

// ---- dynamic thresholding (Imagen 2.3): per-sample order statistics of |x0| by an exact radix select ----------------------------------
// Non-negative fp32 values order as their bit patterns, so the rank-k value of |x0| is found digit by digit over the 31 bits below the
// sign (11 + 10 + 10), most significant first: histogram the digit of every element whose higher bits equal the prefix found so far, walk
// the histogram to the bin that holds the rank, append the bin to the prefix.  No element is stored or moved: x0 is recomputed from
// x / cond / nullp in every pass, by the same kernel (`pass` is a runtime argument, so every pass runs the same instructions and forms the same
// bits).  Two ranks (k_lo, k_hi = k_lo + 1) are carried: while their prefixes agree they share one histogram, from the pass in which they part each
// has its own.  A sample is spread over gridDim.x workgroups; each counts its slice in LDS (integer ds_add, no float atomics) and adds
// its non-empty bins to the sample's histogram in the workspace with integer atomics, so the counts -- and with them the result -- do not
// depend on which workgroup ran when.  The kernel boundary is the barrier between passes: pass p's workgroups each re-derive the prefix from
// pass p - 1's finished histogram (2048 bins, one 8-bin strip per lane), and the finish kernel does it once more and writes lo, hi, s.
// Workspace per sample (unsigned): hist[5][2048] = {pass 0; pass 1 lo, hi; pass 2 lo, hi}, then state[2][4] = {prefix_lo, k_lo, prefix_hi,
// k_hi} on entering pass 1 and pass 2 (written by the sample's first workgroup of pass p, read by pass p + 1).  Zeroed per call.
#define CTQ_BINS 2048
#define CTQ_WS_PER_SAMPLE (5 * CTQ_BINS + 8)
#define CTQ_CHUNK 4096                                       // elements per workgroup: 256 lanes x 4 x 4

// The state on entering `pass` (1, 2, or 3 = finished) -> st[4] in LDS, from the state on entering pass - 1 and that pass's histogram(s).
__device__ inline void ctq_advance(const unsigned* wsb, int pass, unsigned k_lo, unsigned k_hi, unsigned* st, unsigned* wave_tot) {
  unsigned prefix[2] = {0u, 0u}, k[2] = {k_lo, k_hi};
  if (pass > 1) {
    const unsigned* prev = wsb + 5 * CTQ_BINS + (pass - 2) * 4;
    prefix[0] = prev[0]; k[0] = prev[1]; prefix[1] = prev[2]; k[1] = prev[3];
  }
  const int slot_lo = pass == 1 ? 0 : 2 * pass - 3;           // pass - 1's histogram of the low rank: 0, 1, 3
  const int slot[2] = {slot_lo, prefix[0] == prefix[1] ? slot_lo : slot_lo + 1};
  const int bits = pass == 1 ? 11 : 10;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const uint4* h = reinterpret_cast<const uint4*>(wsb + slot[r] * CTQ_BINS + tid * 8);
    const uint4 a = h[0], c = h[1];
    const unsigned bin[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
    unsigned sum = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += bin[e];
    unsigned incl = sum;                                      // inclusive scan over the wave, then over the four waves
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    __syncthreads();                                          // wave_tot of the previous rank has been read
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    unsigned before = incl - sum;
    for (int w = 0; w < wave; ++w) before += wave_tot[w];
    if (k[r] >= before && k[r] - before < sum) {              // exactly one lane: the strip that holds the rank
      unsigned left = k[r] - before;
      int found = -1;
#pragma unroll
      for (int e = 0; e < 8; ++e) {                           // unrolled: bin[] stays in registers
        if (found < 0) { if (left < bin[e]) found = e; else left -= bin[e]; }
      }
      st[2 * r] = (prefix[r] << bits) | (unsigned)(tid * 8 + found);
      st[2 * r + 1] = left;
    }
  }
  __syncthreads();
}

__device__ inline unsigned ctq_key(float x, float cond, float nu, bool guided, float cond_scale, const float* k, int objective) {
  float p = cond;
  if (guided) p = nu + (p - nu) * cond_scale;
  const float x0 = objective == 1 ? ct_start<1>(x, p, k) : objective == 2 ? ct_start<2>(x, p, k) : ct_start<0>(x, p, k);
  return __float_as_uint(x0) & 0x7fffffffu;                   // |x0|: -0.0 is 0, subnormals keep their order
}

__device__ inline void ctq_count(unsigned key, int pass, bool same, const unsigned* st, unsigned (*hist)[CTQ_BINS]) {
  if (pass == 0) { atomicAdd(&hist[0][key >> 20], 1u); return; }
  const unsigned pre = pass == 1 ? key >> 20 : key >> 10;
  const unsigned d = (pass == 1 ? key >> 10 : key) & 1023u;
  if (pre == st[0]) atomicAdd(&hist[0][d], 1u);
  if (!same && pre == st[2]) atomicAdd(&hist[1][d], 1u);
}

// grid (G, B).  VEC: the sample's rows of x, cond and nullp are 16-byte aligned (per_sample % 4 == 0), four elements per lane.
template <bool VEC>
__global__ __launch_bounds__(256) void ct_quantile_pass_kernel(const float* x, const float* cond, const float* nullp, float cond_scale,
                                                               const float* coef, int objective, unsigned k_lo, unsigned k_hi, unsigned* ws,
                                                               long per_sample, int pass) {
  __shared__ unsigned hist[2][CTQ_BINS];
  __shared__ unsigned st[4], wave_tot[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  unsigned* wsb = ws + (long)b * CTQ_WS_PER_SAMPLE;
  if (pass > 0) {
    ctq_advance(wsb, pass, k_lo, k_hi, st, wave_tot);
    if (blockIdx.x == 0 && tid < 4) wsb[5 * CTQ_BINS + (pass - 1) * 4 + tid] = st[tid];
  }
  const bool same = pass == 0 || st[0] == st[2];
  const int bins = pass == 0 ? CTQ_BINS : 1024;
  for (int i = tid; i < bins; i += 256) { hist[0][i] = 0u; hist[1][i] = 0u; }
  __syncthreads();
  const float* k = coef + 13 * b;
  const long base = (long)b * per_sample;
  const bool guided = nullp != nullptr, need_x = objective != 1;
  if (VEC) {
    const long groups = per_sample >> 2;
    for (long g = (long)blockIdx.x * 256 + tid; g < groups; g += (long)gridDim.x * 256) {
      const long i = (base >> 2) + g;
      const f32x4 cv = reinterpret_cast<const f32x4*>(cond)[i];
      f32x4 xv = {0.f, 0.f, 0.f, 0.f}, nv = {0.f, 0.f, 0.f, 0.f};
      if (need_x) xv = reinterpret_cast<const f32x4*>(x)[i];
      if (guided) nv = reinterpret_cast<const f32x4*>(nullp)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) ctq_count(ctq_key(xv[e], cv[e], nv[e], guided, cond_scale, k, objective), pass, same, st, hist);
    }
  } else {
    for (long j = (long)blockIdx.x * 256 + tid; j < per_sample; j += (long)gridDim.x * 256) {
      const long i = base + j;
      ctq_count(ctq_key(need_x ? x[i] : 0.f, cond[i], guided ? nullp[i] : 0.f, guided, cond_scale, k, objective), pass, same, st, hist);
    }
  }
  __syncthreads();
  const int slot = pass == 0 ? 0 : 2 * pass - 1;
  for (int i = tid; i < bins; i += 256) {
    const unsigned h0 = hist[0][i];
    if (h0) atomicAdd(wsb + slot * CTQ_BINS + i, h0);
    if (!same) { const unsigned h1 = hist[1][i]; if (h1) atomicAdd(wsb + (slot + 1) * CTQ_BINS + i, h1); }
  }
}

// grid (B).  out[b] = {lo, hi, s = max(1, lo + (hi - lo) frac)}: two fp32 roundings in the interpolation (no contraction), as a host
// evaluates the same expression on the two values.
__global__ __launch_bounds__(256) void ct_quantile_finish_kernel(const unsigned* ws, unsigned k_lo, unsigned k_hi, float frac, float* out) {
#pragma clang fp contract(off)
  __shared__ unsigned st[4], wave_tot[4];
  const int b = blockIdx.x;
  ctq_advance(ws + (long)b * CTQ_WS_PER_SAMPLE, 3, k_lo, k_hi, st, wave_tot);
  if (threadIdx.x == 0) {
    const float lo = __uint_as_float(st[0]), hi = __uint_as_float(st[2]);
    out[3 * b] = lo; out[3 * b + 1] = hi;
    out[3 * b + 2] = fmaxf(1.f, lo + (hi - lo) * frac);
  }
}

// q_sample and the training target in one pass: x_noisy = alpha x0 + sigma noise; target = noise, x0, or v = alpha noise - sigma x0.
// sched: the sample's schedule row (ld floats apart), alpha and sigma in columns 1 and 2.
__global__ __launch_bounds__(256) void ct_qsample_kernel(const float* x0, const float* noise, const float* sched, int ld, int objective,
                                                         float* x_noisy, float* target, long per_sample, long total) {
  GRID_STRIDE(idx, total) {
    const float* k = sched + (idx / per_sample) * ld;
    const float a = k[1], s = k[2], xs = x0[idx], nz = noise[idx];
    x_noisy[idx] = a * xs + s * nz;
    if (target) target[idx] = objective == 1 ? xs : objective == 2 ? a * nz - s * xs : nz;
  }
}

// ---- masked generation: put the known region back at the iterate's noise level (replacement conditioning) ---------------------------------
// tgt = a known + s noise (two products, one sum, no contraction; a known without noise; known itself without levels), then a select at
// both ends of the mask: m == 0 keeps x, m == 1 takes tgt, anything between is x + m (tgt - x).  The ends being selects, not arithmetic,
// whatever lies under the other end (NaN included) never reaches the result and -0.0 survives.
__device__ inline float inpaint_one(float x, float known, float z, float m, float a, float s, bool levels, bool noisy) {
#pragma clang fp contract(off)
  if (m == 0.f) return x;
  float tgt = known;
  if (levels) {
    tgt = a * known;
    if (noisy) {
      const float sz = s * z;
      tgt = tgt + sz;
    }
  }
  if (m == 1.f) return tgt;
  const float d = tgt - x;
  const float md = m * d;
  return x + md;
}

// grid (chunks of Dch * L, samples); sample b's mask row is mask + b * mask_ld (0: one row for all), broadcast over the Dch channels; its
// levels are coef[b * coef_ld + col_a] and [+ col_s].  VEC: L % 4 == 0 and every buffer (each mask row too) 16-byte aligned, so a group of
// four lies within one row of L; out == x is fine (every lane reads its own elements before it writes them).
template <bool VEC>
__global__ __launch_bounds__(256) void inpaint_blend_kernel(const float* x, const float* known, const float* noise, const float* mask, long mask_ld,
                                                            const float* coef, int coef_ld, int col_a, int col_s, float* out, int B, int L,
                                                            long per_sample) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float a = coef ? coef[(long)b * coef_ld + col_a] : 1.f;
    const float s = (coef && noise) ? coef[(long)b * coef_ld + col_s] : 0.f;
    const float* mrow = mask + b * mask_ld;
    const long base = b * per_sample;
    const bool levels = coef != nullptr, noisy = noise != nullptr;
    if (VEC) {
      const long groups = per_sample >> 2;
      GRID_STRIDE(g, groups) {
        const long i0 = g << 2;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + base + i0), kv = *reinterpret_cast<const f32x4*>(known + base + i0);
        const f32x4 mv = *reinterpret_cast<const f32x4*>(mrow + i0 % L);
        f32x4 zv = {0.f, 0.f, 0.f, 0.f};
        if (levels && noisy) zv = *reinterpret_cast<const f32x4*>(noise + base + i0);
        f32x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = inpaint_one(xv[e], kv[e], zv[e], mv[e], a, s, levels, noisy);
        *reinterpret_cast<f32x4*>(out + base + i0) = ov;
      }
    } else {
      GRID_STRIDE(i, per_sample) {
        const float z = (levels && noisy) ? noise[base + i] : 0.f;
        out[base + i] = inpaint_one(x[base + i], known[base + i], z, mrow[i % L], a, s, levels, noisy);
      }
    }
  }
}

// ---- windowed sampling: cut a song into overlapping windows of the trained length, fuse the window predictions back ----------------------------
// W windows of `window` frames over n >= window frames: window j < W - 1 starts at j * stride, the last one at n - window (clamped: it is
// (W - 1) * stride only when the windows fit exactly), with W = ceil((n - window) / stride) + 1, so (W - 2) * stride < n - window and the
// last window is never one of the regular ones.  Both kernels take that W from a host that has checked it.
__device__ __forceinline__ int window_start(int j, int W, int n, int window, int stride) { return j < W - 1 ? j * stride : n - window; }

// grid (chunks of D * window, window rows); out[r * W + j, d, i] = src[r, d, s_j + i].  VEC: n, window and stride multiples of 4 and both
// buffers 16-byte aligned, so that every start and every row is; a group of four lies within one row of `window`.
template <bool VEC>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* src, float* out, int RW, int W, int D, int n, int window, int stride) {
  const long per_row = (long)D * window;
  for (int rw = blockIdx.y; rw < RW; rw += gridDim.y) {
    const int r = rw / W, j = rw - r * W;
    const float* from = src + (long)r * D * n + window_start(j, W, n, window, stride);
    float* to = out + rw * per_row;
    if (VEC) {
      GRID_STRIDE(g, per_row >> 2) {
        const long i0 = g << 2;
        const long d = i0 / window;
        *reinterpret_cast<f32x4*>(to + i0) = *reinterpret_cast<const f32x4*>(from + d * n + (i0 - d * window));
      }
    } else {
      GRID_STRIDE(i, per_row) {
        const long d = i / window;
        to[i] = from[d * n + (i - d * window)];
      }
    }
  }
}

// The windows that cover frame l, in ascending j: the regular ones j_lo .. j_hi (j * stride <= l < j * stride + window, j <= W - 2; none
// when j_hi < j_lo) and then the last one when l >= n - window.
struct WindowCover { int j_lo, j_hi; bool last; };
__device__ __forceinline__ WindowCover window_cover(int l, int W, int n, int window, int stride) {
  WindowCover c;
  c.j_lo = l >= window ? (l - window) / stride + 1 : 0;
  c.j_hi = min(l / stride, W - 2);
  c.last = l >= n - window;
  return c;
}

// One frame (T = float) or four frames that every window covers alike (T = f32x4) of row `p` = pred + (r * W * D + d) * window, whose
// window j lies at p + j * D * window.  One window: its value, bit for bit.  More: sum_j w p / sum_j w in ascending j, every product
// rounded before its add, one division.
template <typename T>
__device__ __forceinline__ T window_fuse_one(const float* p, const float* weight, long jstep, int l, int W, int n, int window, int stride) {
#pragma clang fp contract(off)
  const WindowCover c = window_cover(l, W, n, window, stride);
  const int regular = c.j_hi >= c.j_lo ? c.j_hi - c.j_lo + 1 : 0;
  const int s_last = n - window;
  if (regular + (c.last ? 1 : 0) == 1) {
    const int j = c.last ? W - 1 : c.j_lo;
    return *reinterpret_cast<const T*>(p + j * jstep + (l - (c.last ? s_last : j * stride)));
  }
  // two windows or more: at least one is regular, and the sums start from it (not from zero: 0 + -0.0 would lose the sign)
  T den = *reinterpret_cast<const T*>(weight + (l - c.j_lo * stride));
  T num = den * *reinterpret_cast<const T*>(p + c.j_lo * jstep + (l - c.j_lo * stride));
  for (int j = c.j_lo + 1; j <= c.j_hi; ++j) {
    const int i = l - j * stride;
    const T w = *reinterpret_cast<const T*>(weight + i);
    const T wp = w * *reinterpret_cast<const T*>(p + j * jstep + i);
    num = num + wp;
    den = den + w;
  }
  if (c.last) {
    const int i = l - s_last;
    const T w = *reinterpret_cast<const T*>(weight + i);
    const T wp = w * *reinterpret_cast<const T*>(p + (W - 1) * jstep + i);
    num = num + wp;
    den = den + w;
  }
  return num / den;
}

// grid (chunks of D * n, R); every output element is written by one lane: no atomics, the same bits on every run.  VEC as in the gather,
// with `weight` aligned too: window boundaries are multiples of 4, so the four frames of a group have the same windows.
template <bool VEC>
__global__ __launch_bounds__(256) void window_fuse_kernel(const float* pred, const float* weight, float* out, int R, int W, int D, int n, int window,
                                                          int stride) {
  const long per_row = (long)D * n, jstep = (long)D * window;
  for (int r = blockIdx.y; r < R; r += gridDim.y) {
    const float* prow = pred + (long)r * W * jstep;
    float* orow = out + r * per_row;
    if (VEC) {
      GRID_STRIDE(g, per_row >> 2) {
        const long i0 = g << 2;
        const long d = i0 / n;
        *reinterpret_cast<f32x4*>(orow + i0) = window_fuse_one<f32x4>(prow + d * window, weight, jstep, (int)(i0 - d * n), W, n, window, stride);
      }
    } else {
      GRID_STRIDE(i, per_row) {
        const long d = i / n;
        orow[i] = window_fuse_one<float>(prow + d * window, weight, jstep, (int)(i - d * n), W, n, window, stride);
      }
    }
  }
}

// ---- classifier-free guidance rescale (Lin et al. 2024, 3.4): the guided prediction brought back to the conditional one's spread ---------------
// out = f_b g, g the guided prediction and f_b = phi sqrt(var_b(cond) / var_b(g)) + (1 - phi), the variances over the sample's per_sample
// values.  Two launches over the same grid (chunks of CFGR_CHUNK elements, samples), no atomics: pass 1 writes every chunk's four sums
// (c, c^2, g, g^2) to ws[b][chunk][4], pass 2 adds a sample's chunks in index order, forms f_b and writes out.  A chunk is a fixed range of
// the sample and a lane's elements and the order of every sum are fixed too, so sample b's bits depend on per_sample and on the path (four-wide
// or scalar) alone, never on B or on which workgroup ran when.  The sums are fp64: sum x^2 - (sum x)^2 / n cancels to (spread / mean)^2 of its
// terms, 1e-4 where the mean is 100 spreads -- beyond fp32, 1e-12 of the variance in fp64.  The squares of fp32 values are exact in fp64.
#define CFGR_CHUNK 4096                                      // elements per workgroup: 256 lanes x 4 x 4

// g in ct_guide's order, every operation rounded (the sum is not contracted with the product): the restatement's bits, whatever the flags.
__device__ inline float cfgr_guide(float cond, float nu, float cond_scale) {
#pragma clang fp contract(off)
  const float d = cond - nu;
  const float m = d * cond_scale;
  return nu + m;
}

__device__ inline void cfgr_add(double (&s)[4], float c, float g) {
#pragma clang fp contract(off)
  const double dc = (double)c, dg = (double)g;
  s[0] += dc; s[1] += dc * dc; s[2] += dg; s[3] += dg * dg;
}

// f_b from the sample's four sums.  1 as a select where there is no spread to rescale to: n < 2, or var(g) <= 0 (all-equal predictions: exact
// zeros give exactly 0; a NaN is not <= 0 and propagates).  A rounding residue below zero in var(cond) counts as zero.
__device__ inline float cfgr_factor(const double (&s)[4], long n, float phi) {
#pragma clang fp contract(off)
  if (n < 2) return 1.f;
  const double dn = (double)n;
  double vc = s[1] - s[0] * s[0] / dn;
  const double vg = s[3] - s[2] * s[2] / dn;
  if (vg <= 0.0) return 1.f;
  if (vc < 0.0) vc = 0.0;
  const double p = (double)phi;
  return (float)(p * sqrt(vc / vg) + (1.0 - p));
}

// grid (G, min(B, 65535)), G = ceil(per_sample / CFGR_CHUNK).  VEC: per_sample % 4 == 0 and cond, nullp (and out, which pass 2 writes) 16-byte
// aligned, so every sample's row is.  Within the wave by shuffles, then the four waves through LDS in wave order.
template <bool VEC>
__global__ __launch_bounds__(256) void cfg_rescale_sums_kernel(const float* cond, const float* nullp, float cond_scale, double* ws, int B,
                                                               long per_sample) {
  __shared__ double part[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long lo = (long)blockIdx.x * CFGR_CHUNK;
  const long hi = lo + CFGR_CHUNK < per_sample ? lo + CFGR_CHUNK : per_sample;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long base = (long)b * per_sample;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (VEC) {
      for (long j = lo + 4 * tid; j < hi; j += 1024) {         // hi is a multiple of 4: the group lies within the chunk
        const f32x4 cv = *reinterpret_cast<const f32x4*>(cond + base + j), nv = *reinterpret_cast<const f32x4*>(nullp + base + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) cfgr_add(s, cv[e], cfgr_guide(cv[e], nv[e], cond_scale));
      }
    } else {
      for (long j = lo + tid; j < hi; j += 256) {
        const float c = cond[base + j];
        cfgr_add(s, c, cfgr_guide(c, nullp[base + j], cond_scale));
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
    }
    if (lane == 0) { part[wave][0] = s[0]; part[wave][1] = s[1]; part[wave][2] = s[2]; part[wave][3] = s[3]; }
    __syncthreads();
    if (tid < 4) ws[((long)b * gridDim.x + blockIdx.x) * 4 + tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    __syncthreads();                                          // part is written again for the next sample
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void cfg_rescale_apply_kernel(const float* cond, const float* nullp, float cond_scale, float phi, const double* ws,
                                                                float* factor, float* out, int B, long per_sample) {
  __shared__ float f_sh;
  const int tid = threadIdx.x;
  const long lo = (long)blockIdx.x * CFGR_CHUNK;
  const long hi = lo + CFGR_CHUNK < per_sample ? lo + CFGR_CHUNK : per_sample;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    if (tid == 0) {                                           // every workgroup of the sample adds the same G rows in the same order
      const double* p = ws + (long)b * gridDim.x * 4;
      double s[4] = {0.0, 0.0, 0.0, 0.0};
      for (unsigned i = 0; i < gridDim.x; ++i) { s[0] += p[4 * i]; s[1] += p[4 * i + 1]; s[2] += p[4 * i + 2]; s[3] += p[4 * i + 3]; }
      const float f = cfgr_factor(s, per_sample, phi);
      f_sh = f;
      if (blockIdx.x == 0) factor[b] = f;
    }
    __syncthreads();
    const float f = f_sh;
    const long base = (long)b * per_sample;
    if (VEC) {
      for (long j = lo + 4 * tid; j < hi; j += 1024) {
        const f32x4 cv = *reinterpret_cast<const f32x4*>(cond + base + j), nv = *reinterpret_cast<const f32x4*>(nullp + base + j);
        f32x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = f * cfgr_guide(cv[e], nv[e], cond_scale);
        *reinterpret_cast<f32x4*>(out + base + j) = ov;
      }
    } else {
      for (long j = lo + tid; j < hi; j += 256) out[base + j] = f * cfgr_guide(cond[base + j], nullp[base + j], cond_scale);
    }
    __syncthreads();                                          // f_sh is written again for the next sample
  }
}

// ---- scaled error norm of an embedded Runge-Kutta step (the adaptive ODE samplers: osufusion_amd/ode.py) --------------------------------------
// ratio[b] = sqrt(mean_i (err_i / tol_i)^2), err = dt sum_j e_j k_j and tol = atol + rtol max(|y0|, |y1|), everything in fp64.  The structure is
// osuf_cfg_rescale's: pass 1 over (chunks of CFGR_CHUNK elements, samples) writes every chunk's sum of terms to ws[b][chunk]; pass 2, one lane
// per sample, adds the sample's chunks in index order and takes the root.  No atomics, a fixed order for every sum: sample b's bits depend on
// per_sample and on the path alone.  Up to nine streams are read once, four floats per lane and stream on the four-wide path; the stage count is a
// template parameter so that every index into the by-value pointer table is a constant and all loads of an element group are issued before
// the first fma.  The host drops the stages whose weight is zero before the launch, as osuf_lincomb's does: they are never read.
struct RkErrArgs { const float* k[7]; double e[7]; };

// (err / tol)^2; 0 as a select where err == 0, so that tol == 0 without an error is no 0 / 0.  The maximum keeps a NaN of either state (fmax
// would drop it).  Every operation is rounded on its own but the chain, which is one fma per stage.
__device__ __forceinline__ double rk_term(double a, double dt, float y0, float y1, double atol, double rtol) {
#pragma clang fp contract(off)
  const double err = dt * a;
  const double m0 = fabs((double)y0), m1 = fabs((double)y1);
  const double m = (m0 > m1 || m0 != m0) ? m0 : m1;
  const double tol = atol + rtol * m;
  const double q = err / tol;
  return err == 0.0 ? 0.0 : q * q;
}

// grid (G, min(B, 65535)), G = ceil(per_sample / CFGR_CHUNK).  VEC: per_sample % 4 == 0 and y0, y1 and every stage read 16-byte aligned.
template <int S, bool VEC>
__global__ __launch_bounds__(256) void rk_error_sums_kernel(const float* y0, const float* y1, RkErrArgs a, double dt, double atol, double rtol,
                                                            double* ws, int B, long per_sample) {
  __shared__ double part[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long lo = (long)blockIdx.x * CFGR_CHUNK;
  const long hi = lo + CFGR_CHUNK < per_sample ? lo + CFGR_CHUNK : per_sample;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long base = (long)b * per_sample;
    double s = 0.0;
    if (VEC) {
      for (long j = lo + 4 * tid; j < hi; j += 1024) {         // hi is a multiple of 4: the group lies within the chunk
        f32x4 kv[S ? S : 1];
#pragma unroll
        for (int st = 0; st < S; ++st) kv[st] = *reinterpret_cast<const f32x4*>(a.k[st] + base + j);
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(y0 + base + j), v1 = *reinterpret_cast<const f32x4*>(y1 + base + j);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double acc = 0.0;
#pragma unroll
          for (int st = 0; st < S; ++st) acc = __builtin_fma(a.e[st], (double)kv[st][c], acc);
          s += rk_term(acc, dt, v0[c], v1[c], atol, rtol);
        }
      }
    } else {
      for (long j = lo + tid; j < hi; j += 256) {
        float kv[S ? S : 1];
#pragma unroll
        for (int st = 0; st < S; ++st) kv[st] = a.k[st][base + j];
        double acc = 0.0;
#pragma unroll
        for (int st = 0; st < S; ++st) acc = __builtin_fma(a.e[st], (double)kv[st], acc);
        s += rk_term(acc, dt, y0[base + j], y1[base + j], atol, rtol);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (tid == 0) ws[(long)b * gridDim.x + blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
    __syncthreads();                                          // part is written again for the next sample
  }
}

// one lane per sample: the G chunk sums in index order, then sqrt(sum / per_sample)
__global__ __launch_bounds__(64) void rk_error_ratio_kernel(const double* ws, double* ratio, int B, long G, long per_sample) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const double* p = ws + (long)b * G;
  double s = 0.0;
  for (long i = 0; i < G; ++i) s += p[i];
  ratio[b] = sqrt(s / (double)per_sample);
}

// ------------------------------------------------------------------------------------------------------------

extern "C" int osuf_axpby_rows(const float* x, const float* y, const float* ca, const float* cb, float* out, int B, long per_sample, hipStream_t stream) {
  if (B <= 0 || per_sample <= 0) return OSUF_EINVAL;
  const long tot = (long)B * per_sample;
  hipLaunchKernelGGL(axpby_rows_kernel, dim3(ew_grid(tot)), dim3(256), 0, stream, x, y, ca, cb, out, per_sample, tot);
  return osuf_launch_status();
}

extern "C" int osuf_ddim_step(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, float* out,
                              int B, long per_sample, hipStream_t stream) {
  if (B <= 0 || per_sample <= 0) return OSUF_EINVAL;
  const long tot = (long)B * per_sample;
  hipLaunchKernelGGL(ddim_step_kernel, dim3(ew_grid(tot)), dim3(256), 0, stream, x, cond, nullp, cond_scale, coef, out, per_sample, tot);
  return osuf_launch_status();
}

extern "C" int osuf_ct_schedule(const float* t, const float* t_next, int kind, float* out, int B, hipStream_t stream) {
  if (B <= 0 || !t || !out || (kind != 0 && kind != 1)) return OSUF_EINVAL;
  hipLaunchKernelGGL(ct_schedule_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, t, t_next, kind, out, B);
  return osuf_launch_status();
}

// One step launch, ancestral (fac, x0_prev and x0 null) or solver; the caller has checked the arguments.  VEC when x, cond and x_next are
// 16-byte aligned and, for the solver, every other buffer that it reads or writes four at a time (NULL is aligned).
template <bool SOLVER, int OBJ, bool THR>
static void ct_step_launch(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, const float* fac,
                           const float* x0_prev, const float* noise, const float* s, long s_ld, float* x_next, float* x0, long per_sample, long tot,
                           hipStream_t stream) {
  const bool rest = !SOLVER || (al16(nullp) && al16(x0_prev) && al16(noise) && al16(x0));
  if (al16(x) && al16(cond) && al16(x_next) && rest && tot >= 4)
    hipLaunchKernelGGL((ct_step_kernel<true, SOLVER, OBJ, THR>), dim3(ew_grid(tot / 4)), dim3(256), 0, stream, x, cond, nullp, cond_scale, coef, fac,
                       x0_prev, noise, s, s_ld, x_next, x0, per_sample, tot);
  else
    hipLaunchKernelGGL((ct_step_kernel<false, SOLVER, OBJ, THR>), dim3(ew_grid(tot)), dim3(256), 0, stream, x, cond, nullp, cond_scale, coef, fac,
                       x0_prev, noise, s, s_ld, x_next, x0, per_sample, tot);
}

// objective (checked: 0 .. 2) and s (the threshold, or NULL) -> the instantiation
template <bool SOLVER>
static int ct_step_dispatch(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, const float* fac,
                            const float* x0_prev, const float* noise, int objective, const float* s, long s_ld, float* x_next, float* x0,
                            long per_sample, long tot, hipStream_t stream) {
#define OSUF_CT_STEP(OBJ)                                                                                                                    \
  do {                                                                                                                                       \
    if (s) ct_step_launch<SOLVER, OBJ, true>(x, cond, nullp, cond_scale, coef, fac, x0_prev, noise, s, s_ld, x_next, x0, per_sample, tot, stream); \
    else ct_step_launch<SOLVER, OBJ, false>(x, cond, nullp, cond_scale, coef, fac, x0_prev, noise, nullptr, 0, x_next, x0, per_sample, tot, stream); \
  } while (0)
  if (objective == OSUF_CT_OBJ_NOISE) OSUF_CT_STEP(0);
  else if (objective == OSUF_CT_OBJ_X_START) OSUF_CT_STEP(1);
  else OSUF_CT_STEP(2);
#undef OSUF_CT_STEP
  return osuf_launch_status();
}

extern "C" int osuf_ct_step_ex(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, const float* noise,
                               int objective, const float* s, long s_ld, float* out, int B, long per_sample, hipStream_t stream) {
  if (B <= 0 || per_sample <= 0 || !x || !cond || !coef || !out || objective < 0 || objective > 2 || (s && s_ld < 1)) return OSUF_EINVAL;
  return ct_step_dispatch<false>(x, cond, nullp, cond_scale, coef, nullptr, nullptr, noise, objective, s, s_ld, out, nullptr, per_sample,
                                 (long)B * per_sample, stream);
}

extern "C" int osuf_ct_step(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, const float* noise,
                            float* out, int B, long per_sample, hipStream_t stream) {
  return osuf_ct_step_ex(x, cond, nullp, cond_scale, coef, noise, OSUF_CT_OBJ_NOISE, nullptr, 0, out, B, per_sample, stream);
}

extern "C" int osuf_ct_solver_schedule(const float* log_snr, int steps, int sampler, float eta, float* rows, float* fac, int B,
                                       hipStream_t stream) {
  if (steps <= 0 || B <= 0 || !log_snr || !rows || !fac || !(eta >= 0.f && eta <= 1.f)) return OSUF_EINVAL;
  if (sampler != OSUF_CT_SAMPLER_DDIM && sampler != OSUF_CT_SAMPLER_DPMPP_2M) return OSUF_EUNSUPPORTED;
  hipLaunchKernelGGL(ct_solver_schedule_kernel, dim3((steps + 255) / 256), dim3(256), 0, stream, log_snr, steps, sampler, eta, rows, fac, B);
  return osuf_launch_status();
}

extern "C" int osuf_ct_solver_step(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, const float* fac,
                                   const float* x0_prev, const float* noise, int objective, const float* s, long s_ld, float* x_next, float* x0,
                                   int B, long per_sample, hipStream_t stream) {
  if (B <= 0 || per_sample <= 0 || !x || !cond || !coef || !fac || !x_next || !x0 || x_next == x0 || objective < 0 || objective > 2 ||
      (s && s_ld < 1))
    return OSUF_EINVAL;
  return ct_step_dispatch<true>(x, cond, nullp, cond_scale, coef, fac, x0_prev, noise, objective, s, s_ld, x_next, x0, per_sample,
                                (long)B * per_sample, stream);
}

extern "C" long osuf_ct_x0_quantile_workspace_bytes(int B) { return B > 0 ? (long)B * CTQ_WS_PER_SAMPLE * (long)sizeof(unsigned) : 0; }

extern "C" int osuf_ct_x0_quantile(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, int objective,
                                   long k_lo, float frac, float* out, void* workspace, int B, long per_sample, hipStream_t stream) {
  if (B <= 0 || B > 65535 || per_sample <= 0 || per_sample > (1L << 30) || !x || !cond || !coef || !out || !workspace || !al16(workspace) ||
      objective < 0 || objective > 2 || k_lo < 0 || k_lo >= per_sample || !(frac >= 0.f && frac <= 1.f))
    return OSUF_EINVAL;
  const unsigned lo = (unsigned)k_lo, hi = (unsigned)(k_lo + 1 < per_sample ? k_lo + 1 : per_sample - 1);
  unsigned* ws = (unsigned*)workspace;
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)osuf_ct_x0_quantile_workspace_bytes(B), stream);
  if (e != hipSuccess) return (int)e;
  // workgroups per sample: CTQ_CHUNK elements each, at most 2048 in the launch (256 CUs x 8), the rest by striding
  long G = (per_sample + CTQ_CHUNK - 1) / CTQ_CHUNK;
  const long cap = 2048 / B > 1 ? 2048 / B : 1;
  if (G > cap) G = cap;
  const bool vec = per_sample % 4 == 0 && al16(x) && al16(cond) && (!nullp || al16(nullp));
  for (int pass = 0; pass < 3; ++pass) {
    if (vec)
      hipLaunchKernelGGL(ct_quantile_pass_kernel<true>, dim3((unsigned)G, B), dim3(256), 0, stream, x, cond, nullp, cond_scale, coef, objective, lo, hi, ws, per_sample, pass);
    else
      hipLaunchKernelGGL(ct_quantile_pass_kernel<false>, dim3((unsigned)G, B), dim3(256), 0, stream, x, cond, nullp, cond_scale, coef, objective, lo, hi, ws, per_sample, pass);
  }
  hipLaunchKernelGGL(ct_quantile_finish_kernel, dim3(B), dim3(256), 0, stream, ws, lo, hi, frac, out);
  return osuf_launch_status();
}

extern "C" int osuf_ct_qsample(const float* x0, const float* noise, const float* sched, int sched_ld, int objective, float* x_noisy,
                               float* target, int B, long per_sample, hipStream_t stream) {
  if (B <= 0 || per_sample <= 0 || !x0 || !noise || !sched || sched_ld < 3 || !x_noisy || objective < 0 || objective > 2) return OSUF_EINVAL;
  const long tot = (long)B * per_sample;
  hipLaunchKernelGGL(ct_qsample_kernel, dim3(ew_grid(tot)), dim3(256), 0, stream, x0, noise, sched, sched_ld, objective, x_noisy, target, per_sample, tot);
  return osuf_launch_status();
}

extern "C" int osuf_inpaint_blend(const float* x, const float* known, const float* noise, const float* mask, long mask_ld, const float* coef,
                                  int coef_ld, int col_a, int col_s, float* out, int B, int Dch, int L, hipStream_t stream) {
  if (!x || !known || !mask || !out || B < 1 || Dch < 1 || L < 1 || mask_ld < 0) return OSUF_EINVAL;
  if (coef && (coef_ld < 1 || col_a < 0 || col_s < 0)) return OSUF_EINVAL;
  const long per_sample = (long)Dch * L;
  const unsigned gy = (unsigned)(B < 65535 ? B : 65535);
  const bool vec = (L & 3) == 0 && (mask_ld & 3) == 0 && al16(x) && al16(known) && al16(mask) && al16(out) && (!noise || !coef || al16(noise));
  if (vec)
    hipLaunchKernelGGL(inpaint_blend_kernel<true>, dim3(ew_grid(per_sample / 4), gy), dim3(256), 0, stream, x, known, noise, mask, mask_ld, coef,
                       coef_ld, col_a, col_s, out, B, L, per_sample);
  else
    hipLaunchKernelGGL(inpaint_blend_kernel<false>, dim3(ew_grid(per_sample), gy), dim3(256), 0, stream, x, known, noise, mask, mask_ld, coef,
                       coef_ld, col_a, col_s, out, B, L, per_sample);
  return osuf_launch_status();
}

// the layout both window entry points accept: n >= window >= stride >= 1 and W the window count of that layout (R * W within an int)
static inline bool bad_windows(int R, int W, int D, int n, int window, int stride) {
  if (R < 1 || W < 1 || D < 1 || n < 1 || window < 1 || stride < 1 || stride > window || n < window) return true;
  return (long)W != ((long)n - window + stride - 1) / stride + 1 || (long)R * W > 0x7fffffffL;
}

extern "C" int osuf_window_gather(const float* src, float* out, int R, int W, int D, int n, int window, int stride, hipStream_t stream) {
  if (!src || !out || bad_windows(R, W, D, n, window, stride)) return OSUF_EINVAL;
  const int RW = R * W;
  const long per_row = (long)D * window;
  const unsigned gy = (unsigned)(RW < 65535 ? RW : 65535);
  const bool vec = ((n | window | stride) & 3) == 0 && al16(src) && al16(out);
  if (vec)
    hipLaunchKernelGGL(window_gather_kernel<true>, dim3(ew_grid(per_row / 4), gy), dim3(256), 0, stream, src, out, RW, W, D, n, window, stride);
  else
    hipLaunchKernelGGL(window_gather_kernel<false>, dim3(ew_grid(per_row), gy), dim3(256), 0, stream, src, out, RW, W, D, n, window, stride);
  return osuf_launch_status();
}

extern "C" int osuf_window_fuse(const float* pred, const float* weight, float* out, int R, int W, int D, int n, int window, int stride,
                                hipStream_t stream) {
  if (!pred || !weight || !out || bad_windows(R, W, D, n, window, stride)) return OSUF_EINVAL;
  const long per_row = (long)D * n;
  const unsigned gy = (unsigned)(R < 65535 ? R : 65535);
  const bool vec = ((n | window | stride) & 3) == 0 && al16(pred) && al16(weight) && al16(out);
  if (vec)
    hipLaunchKernelGGL(window_fuse_kernel<true>, dim3(ew_grid(per_row / 4), gy), dim3(256), 0, stream, pred, weight, out, R, W, D, n, window, stride);
  else
    hipLaunchKernelGGL(window_fuse_kernel<false>, dim3(ew_grid(per_row), gy), dim3(256), 0, stream, pred, weight, out, R, W, D, n, window, stride);
  return osuf_launch_status();
}

static inline long cfgr_chunks(long per_sample) { return (per_sample + CFGR_CHUNK - 1) / CFGR_CHUNK; }

extern "C" long osuf_cfg_rescale_workspace_bytes(int B, long per_sample) {
  return B > 0 && per_sample > 0 ? (long)B * cfgr_chunks(per_sample) * 4 * (long)sizeof(double) : 0;
}

extern "C" int osuf_cfg_rescale(const float* cond, const float* nullp, float cond_scale, float phi, void* ws, float* factor, float* out, int B,
                                long per_sample, hipStream_t stream) {
  if (!cond || !nullp || !ws || !factor || !out || B < 1 || per_sample < 1 || !(phi >= 0.f && phi <= 1.f)) return OSUF_EINVAL;
  const long G = cfgr_chunks(per_sample);
  if ((reinterpret_cast<uintptr_t>(ws) & 7) || G > 0x7fffffffL) return OSUF_EINVAL;
  const dim3 grid((unsigned)G, (unsigned)(B < 65535 ? B : 65535));
  double* sums = (double*)ws;
  if (per_sample % 4 == 0 && al16(cond) && al16(nullp) && al16(out)) {
    hipLaunchKernelGGL(cfg_rescale_sums_kernel<true>, grid, dim3(256), 0, stream, cond, nullp, cond_scale, sums, B, per_sample);
    hipLaunchKernelGGL(cfg_rescale_apply_kernel<true>, grid, dim3(256), 0, stream, cond, nullp, cond_scale, phi, sums, factor, out, B, per_sample);
  } else {
    hipLaunchKernelGGL(cfg_rescale_sums_kernel<false>, grid, dim3(256), 0, stream, cond, nullp, cond_scale, sums, B, per_sample);
    hipLaunchKernelGGL(cfg_rescale_apply_kernel<false>, grid, dim3(256), 0, stream, cond, nullp, cond_scale, phi, sums, factor, out, B, per_sample);
  }
  return osuf_launch_status();
}

extern "C" long osuf_rk_error_workspace_bytes(int B, long per_sample) {
  return B > 0 && per_sample > 0 ? (long)B * cfgr_chunks(per_sample) * (long)sizeof(double) : 0;
}

template <int S>
static void rk_error_launch(const float* y0, const float* y1, const RkErrArgs& a, double dt, double atol, double rtol, double* ws, int B,
                            long per_sample, bool vec, dim3 grid, hipStream_t stream) {
  if (vec) hipLaunchKernelGGL((rk_error_sums_kernel<S, true>), grid, dim3(256), 0, stream, y0, y1, a, dt, atol, rtol, ws, B, per_sample);
  else hipLaunchKernelGGL((rk_error_sums_kernel<S, false>), grid, dim3(256), 0, stream, y0, y1, a, dt, atol, rtol, ws, B, per_sample);
}

static inline bool finite64(double v) { return v - v == 0.0; }

// k, e and step are HOST arrays; step = {dt, atol, rtol}.
extern "C" int osuf_rk_error(const float* y0, const float* y1, const float* const* k, const double* e, int S, const double* step, void* ws,
                             double* ratio, int B, long per_sample, hipStream_t stream) {
  if (!y0 || !y1 || !k || !e || !step || !ws || !ratio || S < 1 || S > 7 || B < 1 || per_sample < 1) return OSUF_EINVAL;
  const double dt = step[0], atol = step[1], rtol = step[2];
  if (!finite64(dt) || !finite64(atol) || !finite64(rtol) || atol < 0.0 || rtol < 0.0 || (atol == 0.0 && rtol == 0.0)) return OSUF_EINVAL;
  const long G = cfgr_chunks(per_sample);
  if ((reinterpret_cast<uintptr_t>(ws) & 7) || G > 0x7fffffffL) return OSUF_EINVAL;
  RkErrArgs a{};
  int used = 0;
  bool vec = per_sample % 4 == 0 && al16(y0) && al16(y1);
  for (int j = 0; j < S; ++j) {
    if (e[j] != e[j]) return OSUF_EINVAL;
    if (e[j] == 0.0) continue;                              // a select: the stage is neither read nor required to exist
    if (!k[j]) return OSUF_EINVAL;
    vec = vec && al16(k[j]);
    a.k[used] = k[j];
    a.e[used++] = e[j];
  }
  const dim3 grid((unsigned)G, (unsigned)(B < 65535 ? B : 65535));
  double* sums = (double*)ws;
  switch (used) {
    case 0: rk_error_launch<0>(y0, y1, a, dt, atol, rtol, sums, B, per_sample, vec, grid, stream); break;
    case 1: rk_error_launch<1>(y0, y1, a, dt, atol, rtol, sums, B, per_sample, vec, grid, stream); break;
    case 2: rk_error_launch<2>(y0, y1, a, dt, atol, rtol, sums, B, per_sample, vec, grid, stream); break;
    case 3: rk_error_launch<3>(y0, y1, a, dt, atol, rtol, sums, B, per_sample, vec, grid, stream); break;
    case 4: rk_error_launch<4>(y0, y1, a, dt, atol, rtol, sums, B, per_sample, vec, grid, stream); break;
    case 5: rk_error_launch<5>(y0, y1, a, dt, atol, rtol, sums, B, per_sample, vec, grid, stream); break;
    case 6: rk_error_launch<6>(y0, y1, a, dt, atol, rtol, sums, B, per_sample, vec, grid, stream); break;
    default: rk_error_launch<7>(y0, y1, a, dt, atol, rtol, sums, B, per_sample, vec, grid, stream); break;
  }
  hipLaunchKernelGGL(rk_error_ratio_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream, (const double*)sums, ratio, B, G, per_sample);
  return osuf_launch_status();
}
