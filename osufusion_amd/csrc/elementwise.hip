// Layout conversion, diffusion-scheduler algebra and optimizer kernels (HBM-bound, 16 B per lane), gfx950.
#include "common.hpp"

#define GRID_STRIDE(idx, total) \
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < (total); idx += (long)gridDim.x * blockDim.x)

// (B, C, L) fp32 channel-major  ->  channels-last rows [B*L][ld] of T, optionally im2col over KT taps:
//   out[b*L + n][t*C + ci] = in[b][ci][n + t - KT/2]   (zero outside [0, L)); columns KT*C .. width-1 are zeroed.
// KT = 1 is a plain transpose (audio stem input); KT = 15 builds the 6-channel x stem's GEMM operand so the
// three CrossEmbed convs (k = 3, 7, 15; unet.py:42-58) become ONE K = 96 GEMM.
template <typename T>
__global__ __launch_bounds__(256) void ncl_to_rows_kernel(const float* in, T* out, long ld, int width, int B, int C, int L, int KT) {
  const int chunks = width >> 3;
  const long total = (long)B * L * chunks;
  GRID_STRIDE(idx, total) {
    // n fastest so the strided reads of `in` coalesce across lanes
    const int n = (int)(idx % L);
    const long r = idx / L;
    const int ch = (int)(r % chunks);
    const int b = (int)(r / chunks);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = ch * 8 + e;
      const int t = col / C, ci = col - t * C;
      const int src = n + t - KT / 2;
      v[e] = (t < KT && src >= 0 && src < L) ? in[((long)b * C + ci) * L + src] : 0.f;
    }
    store8(out + ((long)b * L + n) * ld + ch * 8, v);
  }
}

// rows [B*L][ld] of T (first C columns)  ->  (B, C, L) fp32
template <typename T>
__global__ __launch_bounds__(256) void rows_to_ncl_kernel(const T* in, long ld, float* out, int B, int C, int L) {
  const long total = (long)B * C * L;
  GRID_STRIDE(idx, total) {
    const int n = (int)(idx % L);
    const long r = idx / L;
    const int ci = (int)(r % C);
    const int b = (int)(r / C);
    out[idx] = ElemTraits<T>::load(in + ((long)b * L + n) * ld + ci);
  }
}

// strided 2-D copy with optional dtype change: dst[m][0..cols) = src[m][0..cols)   (cat / slice / cast)
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void copy2d_kernel(const TS* src, long lds_, TD* dst, long ldd, int M, int cols) {
  const int chunks = cols >> 3;
  const long total = (long)M * chunks;
  GRID_STRIDE(idx, total) {
    const long m = idx / chunks;
    const int c = (int)(idx - m * chunks) * 8;
    float v[8];
    load8(src + m * lds_ + c, v);
    store8(dst + m * ldd + c, v);
  }
}

// dst[m][c] = a[m][c] + b[m][c]
template <typename T>
__global__ __launch_bounds__(256) void add2d_kernel(const T* a, long lda, const T* b, long ldb, T* dst, long ldd, int M, int cols) {
  const int chunks = cols >> 3;
  const long total = (long)M * chunks;
  GRID_STRIDE(idx, total) {
    const long m = idx / chunks;
    const int c = (int)(idx - m * chunks) * 8;
    float x[8], y[8];
    load8(a + m * lda + c, x);
    load8(b + m * ldb + c, y);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] += y[e];
    store8(dst + m * ldd + c, x);
  }
}

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

// eps = null + (cond - null) cond_scale;  x0 = clamp((x - sigma eps) / max(alpha, 1e-8), -1, 1);  mean = alpha_next (x (1 - c) / alpha + c x0);
// out = mean + gain * noise.  k = the sample's schedule row.  A zero gain (t_next == 0) or no noise buffer: the mean, whatever noise holds.
// OBJ = what the network predicts (OSUF_CT_OBJ_*): the start prediction is (x - sigma p) / max(alpha, 1e-8) for noise, p itself for x_start and
// alpha x - sigma p for v.  THR: the sample's dynamic threshold s (>= 1, osuf_ct_x0_quantile) replaces the static clamp: clamp(x0, -s, s) / s.
#define OSUF_CT_OBJ_NOISE 0                                  // as in include/osufusion_hip.h
#define OSUF_CT_OBJ_X_START 1
#define OSUF_CT_OBJ_V 2
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

template <int OBJ, bool THR>
__device__ inline float ct_step_one(float x, float cond, const float* nullp, const float* noise, long idx, float cond_scale, const float* k,
                                    const float* s) {
  const float eps = nullp ? ct_guide(cond, nullp[idx], cond_scale) : cond;
  const float x0 = ct_start_clamped<OBJ, THR>(x, eps, k, s);
  const float mean = k[10] * x + k[11] * x0;
  const float gain = k[12];
  return (noise && gain != 0.f) ? mean + gain * noise[idx] : mean;
}

// VEC: x, cond and out are 16-byte aligned, four elements per lane over the flat (B * per_sample) range (a group may straddle two
// samples when per_sample is no multiple of 4: the row is looked up per element there) and a scalar tail of total % 4 elements.
// s (THR only): sample b's threshold is s[b * s_ld], so that column 2 of osuf_ct_x0_quantile's rows is read in place.
template <bool VEC, int OBJ, bool THR>
__global__ __launch_bounds__(256) void ct_step_kernel(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef,
                                                      const float* noise, const float* s, long s_ld, float* out, long per_sample, long total) {
  if (!VEC) {
    GRID_STRIDE(idx, total) {
      const long b = idx / per_sample;
      out[idx] = ct_step_one<OBJ, THR>(x[idx], cond[idx], nullp, noise, idx, cond_scale, coef + 13 * b, THR ? s + b * s_ld : nullptr);
    }
    return;
  }
  const long groups = total >> 2;
  GRID_STRIDE(g, groups) {
    const long i0 = g << 2;
    const long b0 = i0 / per_sample;
    const long left = (b0 + 1) * per_sample - i0;          // elements of this group's first sample from i0 on (>= 1)
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[g], cv = reinterpret_cast<const f32x4*>(cond)[g];
    f32x4 ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long b = e < left ? b0 : (i0 + e) / per_sample;
      ov[e] = ct_step_one<OBJ, THR>(xv[e], cv[e], nullp, noise, i0 + e, cond_scale, coef + 13 * b, THR ? s + b * s_ld : nullptr);
    }
    reinterpret_cast<f32x4*>(out)[g] = ov;
  }
  const long tail = (groups << 2) + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < (total & 3)) {
    const long b = tail / per_sample;
    out[tail] = ct_step_one<OBJ, THR>(x[tail], cond[tail], nullp, noise, tail, cond_scale, coef + 13 * b, THR ? s + b * s_ld : nullptr);
  }
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
#define OSUF_CT_SAMPLER_DDIM 0                               // as in include/osufusion_hip.h
#define OSUF_CT_SAMPLER_DPMPP_2M 1
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

// One element of the solver step.  p = the guided prediction; prev / z are read by the caller only when they enter (k_p != 0, gain != 0).
template <int OBJ, bool THR>
__device__ inline float ct_solver_one(float x, float p, const float* k, const float* s, const float* f, bool use_prev, float prev, bool use_noise,
                                      float z, float* x0_out) {
  const float x0 = ct_start_clamped<OBJ, THR>(x, p, k, s);
  *x0_out = x0;
  float out = f[0] * x + f[1] * x0;
  if (use_prev) out += f[2] * prev;
  if (use_noise) out += f[3] * z;
  return out;
}

// ct_step_kernel's layout (VEC: every buffer that is given is 16-byte aligned; a group of four may straddle two samples; scalar tail) with two
// outputs: x_next and the clamped x0, the next step's x0_prev.  fac = the step's four factors, the same for every sample.
template <bool VEC, int OBJ, bool THR>
__global__ __launch_bounds__(256) void ct_solver_step_kernel(const float* x, const float* cond, const float* nullp, float cond_scale,
                                                             const float* coef, const float* fac, const float* x0_prev, const float* noise,
                                                             const float* s, long s_ld, float* x_next, float* x0, long per_sample, long total) {
  const float f[4] = {fac[0], fac[1], fac[2], fac[3]};
  const bool use_prev = x0_prev && f[2] != 0.f, use_noise = noise && f[3] != 0.f;
  auto scalar = [&](long idx) {
    const long b = idx / per_sample;
    const float p = nullp ? ct_guide(cond[idx], nullp[idx], cond_scale) : cond[idx];
    x_next[idx] = ct_solver_one<OBJ, THR>(x[idx], p, coef + 13 * b, THR ? s + b * s_ld : nullptr, f, use_prev, use_prev ? x0_prev[idx] : 0.f,
                                          use_noise, use_noise ? noise[idx] : 0.f, x0 + idx);
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
    if (nullp) nv = reinterpret_cast<const f32x4*>(nullp)[g];
    if (use_prev) pv = reinterpret_cast<const f32x4*>(x0_prev)[g];
    if (use_noise) zv = reinterpret_cast<const f32x4*>(noise)[g];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long b = e < left ? b0 : (i0 + e) / per_sample;
      const float p = nullp ? ct_guide(cv[e], nv[e], cond_scale) : cv[e];
      float x0e;
      ov[e] = ct_solver_one<OBJ, THR>(xv[e], p, coef + 13 * b, THR ? s + b * s_ld : nullptr, f, use_prev, pv[e], use_noise, zv[e], &x0e);
      sv[e] = x0e;
    }
    reinterpret_cast<f32x4*>(x_next)[g] = ov;
    reinterpret_cast<f32x4*>(x0)[g] = sv;
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

// masked MSE: loss_sum += sum w*(pred-target)^2 (double), grad = 2*w*(pred-target)  (scaled by 1/count later)
// WEIGHTED: w is the length mask times the sample's loss weight wt[b] (min-SNR-gamma); a weight of one leaves every bit as it was.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void mse_kernel(const float* pred, const float* target, const int* orig_len, const float* wt, float* grad,
                                                  double* loss_sum, int Dch, int L, long total) {
  float local = 0.f;
  GRID_STRIDE(idx, total) {
    const int n = (int)(idx % L);
    const long b = idx / ((long)Dch * L);
    float w = (!orig_len || n < orig_len[b]) ? 1.f : 0.f;
    if (WEIGHTED) w *= wt[b];
    const float d = pred[idx] - target[idx];
    local += w * d * d;
    if (grad) grad[idx] = 2.f * w * d;
  }
  local = group_sum<64>(local);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) atomic_add_f64(loss_sum, (double)(red[0] + red[1] + red[2] + red[3]));
}

// ---- optimizer --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sqnorm_kernel(const float* g, long n, double* out) {
  float local = 0.f;
  const long n4 = n >> 2;
  GRID_STRIDE(i, n4) {
    f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
    local += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { float v = g[(n4 << 2) + threadIdx.x]; local += v * v; }
  local = group_sum<64>(local);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) atomic_add_f64(out, (double)(red[0] + red[1] + red[2] + red[3]));
}

// torch.optim.AdamW semantics (decoupled decay), one launch over the flat parameter buffer.
// gscale (device scalar, may be null) multiplies the gradient: 1/world or a clip coefficient, no host sync.
__global__ __launch_bounds__(256) void adamw_kernel(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                                                    float eps, float wd, float inv_bc1, float inv_sqrt_bc2, const float* gscale) {
  const float gs = gscale ? *gscale : 1.f;
  const long n4 = n >> 2;
  GRID_STRIDE(i, n4) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i], gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ge = gv[e] * gs;
      pv[e] *= 1.f - lr * wd;
      mv[e] = beta1 * mv[e] + (1.f - beta1) * ge;
      vv[e] = beta2 * vv[e] + (1.f - beta2) * ge * ge;
      const float denom = sqrtf(vv[e]) * inv_sqrt_bc2 + eps;
      pv[e] -= lr * inv_bc1 * mv[e] / denom;
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    const float ge = g[i] * gs;
    float pe = p[i] * (1.f - lr * wd);
    const float me = beta1 * m[i] + (1.f - beta1) * ge;
    const float ve = beta2 * v[i] + (1.f - beta2) * ge * ge;
    pe -= lr * inv_bc1 * me / (sqrtf(ve) * inv_sqrt_bc2 + eps);
    p[i] = pe; m[i] = me; v[i] = ve;
  }
}

// clip coefficient on device: coef = min(1, max_norm / (sqrt(sumsq) + 1e-6)) * base   (torch clip_grad_norm_ semantics)
__global__ void clip_coef_kernel(const double* sumsq, float max_norm, float base, float* coef, float* total_norm) {
  const float tn = (float)sqrt(*sumsq);
  if (total_norm) *total_norm = tn;
  float c = base;
  if (max_norm > 0.f) c *= fminf(1.f, max_norm / (tn + 1e-6f));
  *coef = c;
}

// fp32 master -> bf16 copy of a flat range (weight packing for linear layers)
__global__ __launch_bounds__(256) void cast_flat_kernel(const float* src, bf16_t* dst, long n) {
  const long n8 = n >> 3;
  GRID_STRIDE(i, n8) {
    float v[8];
    load8(src + i * 8, v);
    store8(dst + i * 8, v);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 7)) { const long i = (n8 << 3) + threadIdx.x; dst[i] = f32_to_bf16(src[i]); }
}

// ------------------------------------------------------------------------------------------------------------

extern "C" int osuf_ncl_to_rows(int dtype, const float* in, void* out, long ld, int width, int B, int C, int L, int KT, hipStream_t stream) {
  if (B <= 0 || C <= 0 || L <= 0 || KT <= 0 || width % 8 || ld % 8 || width < C * KT || width > ld || !al16(out)) return OSUF_EINVAL;
  const long tot = (long)B * L * (width / 8);
  if (dtype == OSUF_DT_BF16) hipLaunchKernelGGL(ncl_to_rows_kernel<bf16_t>, dim3(ew_grid(tot)), dim3(256), 0, stream, in, (bf16_t*)out, ld, width, B, C, L, KT);
  else if (dtype == OSUF_DT_F32) hipLaunchKernelGGL(ncl_to_rows_kernel<float>, dim3(ew_grid(tot)), dim3(256), 0, stream, in, (float*)out, ld, width, B, C, L, KT);
  else return OSUF_EUNSUPPORTED;
  return osuf_launch_status();
}

extern "C" int osuf_rows_to_ncl(int dtype, const void* in, long ld, float* out, int B, int C, int L, hipStream_t stream) {
  if (B <= 0 || C <= 0 || L <= 0 || ld < C) return OSUF_EINVAL;
  const long tot = (long)B * C * L;
  if (dtype == OSUF_DT_BF16) hipLaunchKernelGGL(rows_to_ncl_kernel<bf16_t>, dim3(ew_grid(tot)), dim3(256), 0, stream, (const bf16_t*)in, ld, out, B, C, L);
  else if (dtype == OSUF_DT_F32) hipLaunchKernelGGL(rows_to_ncl_kernel<float>, dim3(ew_grid(tot)), dim3(256), 0, stream, (const float*)in, ld, out, B, C, L);
  else return OSUF_EUNSUPPORTED;
  return osuf_launch_status();
}

extern "C" int osuf_copy2d(int src_dtype, const void* src, long lds_, int dst_dtype, void* dst, long ldd, int M, int cols, hipStream_t stream) {
  if (M <= 0 || cols <= 0 || cols % 8 || lds_ % 8 || ldd % 8 || !al16(src) || !al16(dst)) return OSUF_EINVAL;
  const long tot = (long)M * (cols / 8);
  const dim3 g(ew_grid(tot)), b(256);
  if (src_dtype == OSUF_DT_BF16 && dst_dtype == OSUF_DT_BF16) hipLaunchKernelGGL((copy2d_kernel<bf16_t, bf16_t>), g, b, 0, stream, (const bf16_t*)src, lds_, (bf16_t*)dst, ldd, M, cols);
  else if (src_dtype == OSUF_DT_F32 && dst_dtype == OSUF_DT_F32) hipLaunchKernelGGL((copy2d_kernel<float, float>), g, b, 0, stream, (const float*)src, lds_, (float*)dst, ldd, M, cols);
  else if (src_dtype == OSUF_DT_F32 && dst_dtype == OSUF_DT_BF16) hipLaunchKernelGGL((copy2d_kernel<float, bf16_t>), g, b, 0, stream, (const float*)src, lds_, (bf16_t*)dst, ldd, M, cols);
  else if (src_dtype == OSUF_DT_BF16 && dst_dtype == OSUF_DT_F32) hipLaunchKernelGGL((copy2d_kernel<bf16_t, float>), g, b, 0, stream, (const bf16_t*)src, lds_, (float*)dst, ldd, M, cols);
  else return OSUF_EUNSUPPORTED;
  return osuf_launch_status();
}

extern "C" int osuf_add2d(int dtype, const void* a, long lda, const void* b, long ldb, void* dst, long ldd, int M, int cols, hipStream_t stream) {
  if (M <= 0 || cols <= 0 || cols % 8 || lda % 8 || ldb % 8 || ldd % 8) return OSUF_EINVAL;
  const long tot = (long)M * (cols / 8);
  if (dtype == OSUF_DT_BF16) hipLaunchKernelGGL(add2d_kernel<bf16_t>, dim3(ew_grid(tot)), dim3(256), 0, stream, (const bf16_t*)a, lda, (const bf16_t*)b, ldb, (bf16_t*)dst, ldd, M, cols);
  else if (dtype == OSUF_DT_F32) hipLaunchKernelGGL(add2d_kernel<float>, dim3(ew_grid(tot)), dim3(256), 0, stream, (const float*)a, lda, (const float*)b, ldb, (float*)dst, ldd, M, cols);
  else return OSUF_EUNSUPPORTED;
  return osuf_launch_status();
}

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

template <int OBJ, bool THR>
static void ct_step_launch(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, const float* noise,
                           const float* s, long s_ld, float* out, long per_sample, long tot, hipStream_t stream) {
  if (al16(x) && al16(cond) && al16(out) && tot >= 4)
    hipLaunchKernelGGL((ct_step_kernel<true, OBJ, THR>), dim3(ew_grid(tot / 4)), dim3(256), 0, stream, x, cond, nullp, cond_scale, coef, noise, s,
                       s_ld, out, per_sample, tot);
  else
    hipLaunchKernelGGL((ct_step_kernel<false, OBJ, THR>), dim3(ew_grid(tot)), dim3(256), 0, stream, x, cond, nullp, cond_scale, coef, noise, s,
                       s_ld, out, per_sample, tot);
}

extern "C" int osuf_ct_step_ex(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, const float* noise,
                               int objective, const float* s, long s_ld, float* out, int B, long per_sample, hipStream_t stream) {
  if (B <= 0 || per_sample <= 0 || !x || !cond || !coef || !out || objective < 0 || objective > 2 || (s && s_ld < 1)) return OSUF_EINVAL;
  const long tot = (long)B * per_sample;
#define OSUF_CT_STEP(OBJ)                                                                                                      \
  do {                                                                                                                         \
    if (s) ct_step_launch<OBJ, true>(x, cond, nullp, cond_scale, coef, noise, s, s_ld, out, per_sample, tot, stream);           \
    else ct_step_launch<OBJ, false>(x, cond, nullp, cond_scale, coef, noise, nullptr, 0, out, per_sample, tot, stream);         \
  } while (0)
  if (objective == OSUF_CT_OBJ_NOISE) OSUF_CT_STEP(0);
  else if (objective == OSUF_CT_OBJ_X_START) OSUF_CT_STEP(1);
  else OSUF_CT_STEP(2);
#undef OSUF_CT_STEP
  return osuf_launch_status();
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

template <int OBJ, bool THR>
static void ct_solver_step_launch(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, const float* fac,
                                  const float* x0_prev, const float* noise, const float* s, long s_ld, float* x_next, float* x0, long per_sample,
                                  long tot, hipStream_t stream) {
  if (al16(x) && al16(cond) && al16(nullp) && al16(x0_prev) && al16(noise) && al16(x_next) && al16(x0) && tot >= 4)      // NULL is aligned
    hipLaunchKernelGGL((ct_solver_step_kernel<true, OBJ, THR>), dim3(ew_grid(tot / 4)), dim3(256), 0, stream, x, cond, nullp, cond_scale, coef, fac,
                       x0_prev, noise, s, s_ld, x_next, x0, per_sample, tot);
  else
    hipLaunchKernelGGL((ct_solver_step_kernel<false, OBJ, THR>), dim3(ew_grid(tot)), dim3(256), 0, stream, x, cond, nullp, cond_scale, coef, fac,
                       x0_prev, noise, s, s_ld, x_next, x0, per_sample, tot);
}

extern "C" int osuf_ct_solver_step(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, const float* fac,
                                   const float* x0_prev, const float* noise, int objective, const float* s, long s_ld, float* x_next, float* x0,
                                   int B, long per_sample, hipStream_t stream) {
  if (B <= 0 || per_sample <= 0 || !x || !cond || !coef || !fac || !x_next || !x0 || x_next == x0 || objective < 0 || objective > 2 ||
      (s && s_ld < 1))
    return OSUF_EINVAL;
  const long tot = (long)B * per_sample;
#define OSUF_CT_SOLVER_STEP(OBJ)                                                                                                            \
  do {                                                                                                                                      \
    if (s) ct_solver_step_launch<OBJ, true>(x, cond, nullp, cond_scale, coef, fac, x0_prev, noise, s, s_ld, x_next, x0, per_sample, tot, stream); \
    else ct_solver_step_launch<OBJ, false>(x, cond, nullp, cond_scale, coef, fac, x0_prev, noise, nullptr, 0, x_next, x0, per_sample, tot, stream); \
  } while (0)
  if (objective == OSUF_CT_OBJ_NOISE) OSUF_CT_SOLVER_STEP(0);
  else if (objective == OSUF_CT_OBJ_X_START) OSUF_CT_SOLVER_STEP(1);
  else OSUF_CT_SOLVER_STEP(2);
#undef OSUF_CT_SOLVER_STEP
  return osuf_launch_status();
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

extern "C" int osuf_mse(const float* pred, const float* target, const int* orig_len, float* grad, double* loss_sum, int B, int Dch, int L,
                        hipStream_t stream) {
  if (B <= 0 || Dch <= 0 || L <= 0) return OSUF_EINVAL;
  const long tot = (long)B * Dch * L;
  hipLaunchKernelGGL(mse_kernel<false>, dim3(ew_grid(tot)), dim3(256), 0, stream, pred, target, orig_len, nullptr, grad, loss_sum, Dch, L, tot);
  return osuf_launch_status();
}

extern "C" int osuf_mse_w(const float* pred, const float* target, const int* orig_len, const float* w, float* grad, double* loss_sum, int B,
                          int Dch, int L, hipStream_t stream) {
  if (B <= 0 || Dch <= 0 || L <= 0 || !w) return OSUF_EINVAL;
  const long tot = (long)B * Dch * L;
  hipLaunchKernelGGL(mse_kernel<true>, dim3(ew_grid(tot)), dim3(256), 0, stream, pred, target, orig_len, w, grad, loss_sum, Dch, L, tot);
  return osuf_launch_status();
}

extern "C" int osuf_sqnorm(const float* g, long n, double* out, hipStream_t stream) {
  if (n <= 0 || !al16(g)) return OSUF_EINVAL;
  hipLaunchKernelGGL(sqnorm_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, stream, g, n, out);
  return osuf_launch_status();
}

extern "C" int osuf_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, float wd,
                          int step, const float* gscale, hipStream_t stream) {
  if (n <= 0 || step <= 0 || !al16(p) || !al16(g) || !al16(m) || !al16(v)) return OSUF_EINVAL;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adamw_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, stream, p, g, m, v, n, lr, beta1, beta2, eps, wd,
                     (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2)), gscale);
  return osuf_launch_status();
}

extern "C" int osuf_clip_coef(const double* sumsq, float max_norm, float base, float* coef, float* total_norm, hipStream_t stream) {
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(1), 0, stream, sumsq, max_norm, base, coef, total_norm);
  return osuf_launch_status();
}

extern "C" int osuf_cast_f32_bf16(const float* src, void* dst, long n, hipStream_t stream) {
  if (n <= 0 || !al16(src) || !al16(dst)) return OSUF_EINVAL;
  hipLaunchKernelGGL(cast_flat_kernel, dim3(ew_grid(n / 8 + 1)), dim3(256), 0, stream, src, (bf16_t*)dst, n);
  return osuf_launch_status();
}

// ------------------------------------------------------------------------------------------------------
// Weight packing: fp32 master (O, I, k) [torch Conv1d / Linear layout] -> the two GEMM operand layouts in ONE pass:
//   fwd   F[t][o][i]  = w[o][i][t]
//   dgrad D[t'][i][o] : kind 0 (same)  t' < k : w[o][i][k-1-t']                     (flipped taps)
//                       kind 1 (down)  4 taps : w[..][0], w[..][1], w[..][2], w[..][2]   (tap 3 = reflected column)
//                       kind 2 (up)    4 taps : w2, w1+w2, w0+w1, w0                 (nearest-x2 + k3 as a stride-2 conv over dy)
// (the torch path did permute + cast + contiguous (+ flip / cat) per layout: ~1.4 k small launches and ~9 ms of a 295 ms step)
// One 32x32 (o, i) tile per block, up to 4 taps at a time through LDS so both outputs are written with contiguous rows.
// ------------------------------------------------------------------------------------------------------
// ADAPT: the packed value is the LoRA / DoRA effective weight g[o] * (w + s * sum_q B[o][q] A[q][i][t]) (q ascending, fp32 FMA chain),
// formed on the fly from the frozen master and the rank-r factors -- the full-size fp32 effective weight is never materialised.
struct AdaptArgs { const float* A; const float* B; const float* g; float s; int r; };

// lora_A / lora_B slabs of one 32 x 32 (o, i) tile -> LDS: As[q][i_local * k + t], Bs[o_local][q], gs[o_local]
__device__ __forceinline__ void stage_adapter(const AdaptArgs& ad, float* As, float* Bs, float* gs, int O, int I, int k, int o0, int i0) {
  const int wk = 32 * k;
  for (int e = threadIdx.x; e < ad.r * wk; e += 256) {
    const int q = e / wk, c = e - q * wk;
    As[e] = (i0 * k + c < I * k) ? ad.A[(long)q * I * k + (long)i0 * k + c] : 0.f;
  }
  for (int e = threadIdx.x; e < 32 * ad.r; e += 256) Bs[e] = (o0 + e / ad.r < O) ? ad.B[(long)o0 * ad.r + e] : 0.f;
  if (threadIdx.x < 32) gs[threadIdx.x] = (ad.g && o0 + threadIdx.x < O) ? ad.g[o0 + threadIdx.x] : 1.f;
  __syncthreads();
}

__device__ __forceinline__ float adapted_value(const AdaptArgs& ad, const float* As, const float* Bs, int k, int row, int col, int t, float w) {
  float acc = 0.f;
  const float* a = As + col * k + t;
  const float* b = Bs + row * ad.r;
  for (int q = 0; q < ad.r; ++q) acc = fmaf(b[q], a[q * 32 * k], acc);
  return fmaf(ad.s, acc, w);
}

template <typename TO, bool ADAPT>
__device__ __forceinline__ void pack_tile(const float* __restrict__ w, int O, int I, int k, TO* F, long f_ld, long f_ts, TO* D, long d_ld, long d_ts,
                                          int dkind, const AdaptArgs& ad, int o0, int i0, float (*tile)[32][33], float* adapt_lds) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  float* As = adapt_lds;
  float* Bs = As + (ADAPT ? ad.r * 32 * k : 0);
  float* gs = Bs + (ADAPT ? 32 * ad.r : 0);
  if constexpr (ADAPT) stage_adapter(ad, As, Bs, gs, O, I, k, o0, i0);
  for (int t0 = 0; t0 < k; t0 += 4) {
    const int nt = min(4, k - t0);
    for (int r = ty; r < 32; r += 8) {
      const int o = o0 + r, i = i0 + tx;
      if (o < O && i < I) {
        const float* src = w + ((long)o * I + i) * k + t0;
        for (int t = 0; t < nt; ++t) {
          float v = src[t];
          if constexpr (ADAPT) v = gs[r] * adapted_value(ad, As, Bs, k, r, tx, t0 + t, v);
          tile[t][r][tx] = v;
          if (F) ElemTraits<TO>::store(F + (long)(t0 + t) * f_ts + (long)o * f_ld + i, v);
        }
      }
    }
    __syncthreads();
    if (D) {
      for (int r = ty; r < 32; r += 8) {
        const int i = i0 + r, o = o0 + tx;                  // tile[t][o_local = tx][i_local = r]
        if (o < O && i < I) {
          TO* dst = D + (long)i * d_ld + o;
          if (dkind == 0) {
            for (int t = 0; t < nt; ++t) ElemTraits<TO>::store(dst + (long)(k - 1 - (t0 + t)) * d_ts, tile[t][tx][r]);
          } else if (dkind == 1) {
            const float w0 = tile[0][tx][r], w1 = tile[1][tx][r], w2 = tile[2][tx][r];
            ElemTraits<TO>::store(dst, w0); ElemTraits<TO>::store(dst + d_ts, w1);
            ElemTraits<TO>::store(dst + 2 * d_ts, w2); ElemTraits<TO>::store(dst + 3 * d_ts, w2);
          } else {
            const float w0 = tile[0][tx][r], w1 = tile[1][tx][r], w2 = tile[2][tx][r];
            ElemTraits<TO>::store(dst, w2); ElemTraits<TO>::store(dst + d_ts, w1 + w2);
            ElemTraits<TO>::store(dst + 2 * d_ts, w0 + w1); ElemTraits<TO>::store(dst + 3 * d_ts, w0);
          }
        }
      }
    }
    __syncthreads();
  }
}

template <typename TO, bool ADAPT>
__global__ __launch_bounds__(256) void pack_weight_kernel(const float* __restrict__ w, int O, int I, int k, TO* F, long f_ld, long f_ts, TO* D,
                                                          long d_ld, long d_ts, int dkind, AdaptArgs ad) {
  __shared__ float tile[4][32][33];
  extern __shared__ float adapt_lds[];                      // ADAPT: As | Bs | gs
  pack_tile<TO, ADAPT>(w, O, I, k, F, f_ld, f_ts, D, d_ld, d_ts, dkind, ad, blockIdx.y * 32, blockIdx.x * 32, tile, adapt_lds);
}

// Every plain (un-adapted) weight of the model in ONE launch: block b serves the descriptor whose [block0, block0 + bx*by) range holds
// it (binary search over the table), then runs the tile body above.  After an optimizer step all ~320 packed operands are stale at
// once; one launch per weight was 318 launches and 2.05 ms per step, most of it launch gaps and partly filled grids.
template <typename TO>
__global__ __launch_bounds__(256) void pack_weight_group_kernel(const osuf_pack_desc* __restrict__ descs, int n) {
  __shared__ float tile[4][32][33];
  const int bid = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {                                        // last descriptor with block0 <= bid (uniform per block)
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].block0 <= bid) lo = mid; else hi = mid - 1;
  }
  const osuf_pack_desc d = descs[lo];
  const int local = bid - d.block0;
  const int bx = (d.I + 31) / 32;
  if (local >= bx * ((d.O + 31) / 32)) return;             // uniform: before any barrier
  const AdaptArgs none{nullptr, nullptr, nullptr, 0.f, 0};
  pack_tile<TO, false>(d.w, d.O, d.I, d.k, (TO*)d.F, d.f_ld, d.f_tapstride, (TO*)d.D, d.d_ld, d.d_tapstride, d.dkind, none,
                       (local / bx) * 32, (local % bx) * 32, tile, nullptr);
}

extern "C" int osuf_pack_weight(const float* w, int O, int I, int k, int out_dtype, void* F, long f_ld, long f_tapstride, void* D, long d_ld,
                                long d_tapstride, int dkind, hipStream_t stream) {
  if (!w || O <= 0 || I <= 0 || k <= 0 || dkind < 0 || dkind > 2 || (dkind != 0 && k != 3) || (!F && !D)) return OSUF_EINVAL;
  dim3 grid((I + 31) / 32, (O + 31) / 32);
  const AdaptArgs none{nullptr, nullptr, nullptr, 0.f, 0};
  if (out_dtype == OSUF_DT_BF16)
    hipLaunchKernelGGL((pack_weight_kernel<bf16_t, false>), grid, dim3(256), 0, stream, w, O, I, k, (bf16_t*)F, f_ld, f_tapstride, (bf16_t*)D, d_ld, d_tapstride, dkind, none);
  else if (out_dtype == OSUF_DT_F32)
    hipLaunchKernelGGL((pack_weight_kernel<float, false>), grid, dim3(256), 0, stream, w, O, I, k, (float*)F, f_ld, f_tapstride, (float*)D, d_ld, d_tapstride, dkind, none);
  else return OSUF_EUNSUPPORTED;
  return osuf_launch_status();
}

// descs: DEVICE array of n osuf_pack_desc whose block0 fields are the running sum of ceil(O/32)*ceil(I/32) (ascending, descs[0].block0 = 0);
// total_blocks = that sum over all n.  All outputs share out_dtype.
extern "C" int osuf_pack_weight_group(const osuf_pack_desc* descs, int n, int total_blocks, int out_dtype, hipStream_t stream) {
  if (!descs || n <= 0 || total_blocks <= 0) return OSUF_EINVAL;
  if (out_dtype == OSUF_DT_BF16) hipLaunchKernelGGL(pack_weight_group_kernel<bf16_t>, dim3(total_blocks), dim3(256), 0, stream, descs, n);
  else if (out_dtype == OSUF_DT_F32) hipLaunchKernelGGL(pack_weight_group_kernel<float>, dim3(total_blocks), dim3(256), 0, stream, descs, n);
  else return OSUF_EUNSUPPORTED;
  return osuf_launch_status();
}

// The same two layouts of the LoRA / DoRA effective weight (see AdaptArgs): A (r, I, k), B (O, r), g (O) or NULL (= 1).
extern "C" int osuf_pack_weight_adapted(const float* w, const float* A, const float* B, const float* g, float scaling, int r, int O, int I, int k,
                                        int out_dtype, void* F, long f_ld, long f_tapstride, void* D, long d_ld, long d_tapstride, int dkind,
                                        hipStream_t stream) {
  if (!w || !A || !B || r <= 0 || O <= 0 || I <= 0 || k <= 0 || dkind < 0 || dkind > 2 || (dkind != 0 && k != 3) || (!F && !D)) return OSUF_EINVAL;
  const size_t lds = ((size_t)r * 32 * k + 32 * r + 32) * sizeof(float);
  if (lds > 96 * 1024) return OSUF_EUNSUPPORTED;
  dim3 grid((I + 31) / 32, (O + 31) / 32);
  const AdaptArgs ad{A, B, g, scaling, r};
  if (out_dtype == OSUF_DT_BF16) {
    if (lds > 32 * 1024) (void)hipFuncSetAttribute((const void*)pack_weight_kernel<bf16_t, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((pack_weight_kernel<bf16_t, true>), grid, dim3(256), lds, stream, w, O, I, k, (bf16_t*)F, f_ld, f_tapstride, (bf16_t*)D, d_ld, d_tapstride, dkind, ad);
  } else if (out_dtype == OSUF_DT_F32) {
    if (lds > 32 * 1024) (void)hipFuncSetAttribute((const void*)pack_weight_kernel<float, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((pack_weight_kernel<float, true>), grid, dim3(256), lds, stream, w, O, I, k, (float*)F, f_ld, f_tapstride, (float*)D, d_ld, d_tapstride, dkind, ad);
  } else return OSUF_EUNSUPPORTED;
  return osuf_launch_status();
}

// DoRA gain g[o] = mag[o] / ||W[o] + s (BA)[o]||_2 without forming the row anywhere: per-tile partial sums of squares
// (partial[i_tile][o], fixed order -> deterministic), then one thread per output channel finishes g and writes the
// transposed rank-r operand (s g B)^T = [r][O] that the adapter-gradient GEMM du = dy (s g B) consumes, in f32 and bf16.
__global__ __launch_bounds__(256) void dora_sumsq_kernel(const float* __restrict__ w, int O, int I, int k, AdaptArgs ad, float* __restrict__ partial) {
  extern __shared__ float adapt_lds[];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int o0 = blockIdx.y * 32, i0 = blockIdx.x * 32;
  float* As = adapt_lds;
  float* Bs = As + ad.r * 32 * k;
  float* gs = Bs + 32 * ad.r;
  stage_adapter(ad, As, Bs, gs, O, I, k, o0, i0);
  for (int r = ty; r < 32; r += 8) {
    const int o = o0 + r, i = i0 + tx;
    float ss = 0.f;
    if (o < O && i < I) {
      const float* src = w + ((long)o * I + i) * k;
      for (int t = 0; t < k; ++t) {
        const float v = adapted_value(ad, As, Bs, k, r, tx, t, src[t]);
        ss = fmaf(v, v, ss);
      }
    }
    ss = group_sum<32>(ss);
    if (tx == 0 && o < O) partial[(long)blockIdx.x * O + o] = ss;
  }
}

__global__ __launch_bounds__(256) void dora_gain_kernel(const float* __restrict__ partial, int ntiles, const float* __restrict__ mag,
                                                        const float* __restrict__ Bm, int O, int r, float s, float* __restrict__ g_out,
                                                        float* __restrict__ sgbt32, bf16_t* __restrict__ sgbt16) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= O) return;
  float g = 1.f;
  if (mag) {
    float ss = 0.f;
    for (int t = 0; t < ntiles; ++t) ss += partial[(long)t * O + o];
    g = mag[o] / sqrtf(ss);
  }
  g_out[o] = g;
  for (int q = 0; q < r; ++q) {
    const float v = s * g * Bm[(long)o * r + q];
    if (sgbt32) sgbt32[(long)q * O + o] = v;
    if (sgbt16) sgbt16[(long)q * O + o] = f32_to_bf16(v);
  }
}

extern "C" int osuf_dora_gain(const float* W, const float* A, const float* B, const float* mag, int O, int I, int k, int r, float scaling,
                              float* partial, float* g, float* sgbt32, void* sgbt16, hipStream_t stream) {
  if (!W || !A || !B || !g || O <= 0 || I <= 0 || k <= 0 || r <= 0 || (mag && !partial)) return OSUF_EINVAL;
  const int ntiles = (I + 31) / 32;
  if (mag) {
    const size_t lds = ((size_t)r * 32 * k + 32 * r + 32) * sizeof(float);
    if (lds > 96 * 1024) return OSUF_EUNSUPPORTED;
    if (lds > 32 * 1024) (void)hipFuncSetAttribute((const void*)dora_sumsq_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const AdaptArgs ad{A, B, nullptr, scaling, r};
    hipLaunchKernelGGL(dora_sumsq_kernel, dim3(ntiles, (O + 31) / 32), dim3(256), lds, stream, W, O, I, k, ad, partial);
  }
  hipLaunchKernelGGL(dora_gain_kernel, dim3((O + 255) / 256), dim3(256), 0, stream, partial, ntiles, mag, B, O, r, scaling, g, sgbt32, (bf16_t*)sgbt16);
  return osuf_launch_status();
}

// ------------------------------------------------------------------------------------------------------
// LoRA / DoRA effective weight (modules/lora_layers.py:16-26,72-92; peft 0.12 DoraLinearLayer):
//   V[o][j]   = W[o][j] + s * sum_r B[o][r] * A[r][j]           j over (in, tap), r ascending, fp32 FMA chain
//   DoRA:  g[o] = m[o] / ||V[o][:]||_2 ,  Weff = g[o] * V        (the norm is a constant of the step: detached in the reference)
//   LoRA:  g[o] = 1 ,                     Weff = V
// so that  base(x) + (g-1)*conv(x,W) + g*s*B(A(x))  ==  conv(x, Weff) + bias  -- the forward and the input gradient then run
// the unchanged conv / linear GEMMs on Weff; only the adapter gradients use the factored form (functional.adapter_grads).
// One block per output channel; the row lives in LDS between the norm and the scale pass.
// ------------------------------------------------------------------------------------------------------
template <int OC>
__global__ __launch_bounds__(256) void dora_effective_kernel(const float* __restrict__ W, const float* __restrict__ A, const float* __restrict__ Bm,
                                                             const float* __restrict__ mag, int O, int IK, int r, float s, float* __restrict__ Weff,
                                                             float* __restrict__ g_out) {
  // OC output channels per block: every lora_A element fetched from L2 serves OC rows (with one row per block the r x IK matrix was
  // re-read by every output channel: r * |W| * 4 B of L2 traffic per adapted layer, 5.9 ms of a LoRA step)
  extern __shared__ float rows[];                           // [OC][IK]
  __shared__ float part[OC][4];
  const int o0 = blockIdx.x * OC, tid = threadIdx.x;
  float ss[OC];
#pragma unroll
  for (int c = 0; c < OC; ++c) ss[c] = 0.f;
  for (int j = tid; j < IK; j += 256) {
    float acc[OC];
#pragma unroll
    for (int c = 0; c < OC; ++c) acc[c] = 0.f;
    for (int q = 0; q < r; ++q) {
      const float av = A[(long)q * IK + j];
#pragma unroll
      for (int c = 0; c < OC; ++c) {
        const int o = min(o0 + c, O - 1);
        acc[c] = fmaf(Bm[(long)o * r + q], av, acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < OC; ++c) {
      const int o = min(o0 + c, O - 1);
      const float v = fmaf(s, acc[c], W[(long)o * IK + j]);
      rows[c * IK + j] = v;
      ss[c] = fmaf(v, v, ss[c]);
    }
  }
  float g[OC];
#pragma unroll
  for (int c = 0; c < OC; ++c) g[c] = 1.f;
  if (mag) {
#pragma unroll
    for (int c = 0; c < OC; ++c) {
      const float t = group_sum<64>(ss[c]);
      if ((tid & 63) == 0) part[c][tid >> 6] = t;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < OC; ++c) {
      const int o = min(o0 + c, O - 1);
      g[c] = mag[o] / sqrtf(part[c][0] + part[c][1] + part[c][2] + part[c][3]);
    }
  }
  if (tid < OC && o0 + tid < O && g_out) {
    float gv = 1.f;
#pragma unroll
    for (int c = 0; c < OC; ++c) if (c == tid) gv = g[c];
    g_out[o0 + tid] = gv;
  }
  for (int j = tid; j < IK; j += 256) {                    // each thread re-reads only what it wrote
#pragma unroll
    for (int c = 0; c < OC; ++c)
      if (o0 + c < O) Weff[(long)(o0 + c) * IK + j] = g[c] * rows[c * IK + j];
  }
}

extern "C" int osuf_dora_effective(const float* W, const float* A, const float* B, const float* mag, int O, int IK, int r, float scaling,
                                   float* Weff, float* g, hipStream_t stream) {
  if (!W || !A || !B || !Weff || O <= 0 || IK <= 0 || r <= 0 || (long)IK * 4 > 150 * 1024) return OSUF_EINVAL;
  // as many channels per block as fit ~96 KiB of LDS (8, 4, 2 or 1)
  const long row_bytes = (long)IK * 4;
  const int oc = row_bytes * 8 <= 96 * 1024 ? 8 : row_bytes * 4 <= 96 * 1024 ? 4 : row_bytes * 2 <= 96 * 1024 ? 2 : 1;
  const int lds = (int)(row_bytes * oc);
  const dim3 grid((O + oc - 1) / oc);
#define OSUF_DORA_LAUNCH(OCV)                                                                                                         \
  do {                                                                                                                                \
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)dora_effective_kernel<OCV>, hipFuncAttributeMaxDynamicSharedMemorySize, lds); \
    hipLaunchKernelGGL(dora_effective_kernel<OCV>, grid, dim3(256), lds, stream, W, A, B, mag, O, IK, r, scaling, Weff, g);           \
  } while (0)
  if (oc == 8) OSUF_DORA_LAUNCH(8);
  else if (oc == 4) OSUF_DORA_LAUNCH(4);
  else if (oc == 2) OSUF_DORA_LAUNCH(2);
  else OSUF_DORA_LAUNCH(1);
#undef OSUF_DORA_LAUNCH
  return osuf_launch_status();
}

// Tail of the adapter gradients (functional.adapter_grads), one launch instead of ~10 small torch kernels per adapted layer:
//   dB[o][q]    (+)= sg[o] * tb[o][q]                      tb = dy^T u, sg = s * g
//   dA[q][i][t] (+)= gt[k-1-t][i][q]                       gt = the swapped, tap-flipped wgrad x^T du (rank-r operand second)
//   dm[o]       (+)= (s0[o] - bias[o] * s1[o]) / m[o]      s0 = sum_m dy*y, s1 = sum_m dy   (dm / bias may be NULL)
__global__ __launch_bounds__(256) void adapter_finish_kernel(const float* __restrict__ tb, const float* __restrict__ sg, float* dB,
                                                             const float* __restrict__ gt, float* dA, const float* __restrict__ s0,
                                                             const float* __restrict__ s1, const float* __restrict__ bias,
                                                             const float* __restrict__ m, float* dm, int O, int I, int k, int r, int acc) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx < (long)O * r) {
    const float v = sg[idx / r] * tb[idx];
    dB[idx] = acc ? dB[idx] + v : v;
  }
  if (idx < (long)r * I * k) {
    const int q = (int)(idx / ((long)I * k));
    const int rem = (int)(idx - (long)q * I * k);
    const int i = rem / k, t = rem - i * k;
    const float v = gt[((long)(k - 1 - t) * I + i) * r + q];
    dA[idx] = acc ? dA[idx] + v : v;
  }
  if (dm && idx < O) {
    const float v = (s0[idx] - (bias ? bias[idx] * s1[idx] : 0.f)) / m[idx];
    dm[idx] = acc ? dm[idx] + v : v;
  }
}

extern "C" int osuf_adapter_finish(const float* tb, const float* sg, float* dB, const float* gt, float* dA, const float* s0, const float* s1,
                                   const float* bias, const float* m, float* dm, int O, int I, int k, int r, int accumulate,
                                   hipStream_t stream) {
  if (!tb || !sg || !dB || !gt || !dA || O <= 0 || I <= 0 || k <= 0 || r <= 0 || (dm && (!s0 || !m || (bias && !s1)))) return OSUF_EINVAL;
  long n = (long)O * r;
  if ((long)r * I * k > n) n = (long)r * I * k;
  if (O > n) n = O;
  hipLaunchKernelGGL(adapter_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tb, sg, dB, gt, dA, s0, s1, bias, m, dm, O, I,
                     k, r, accumulate);
  return osuf_launch_status();
}

// ------------------------------------------------------------------------------------------------------
// Clock probe (tools/clock_probe.py): every wave runs `iters` x 8 independent v_mfma_f32_32x32x16_bf16 back to back (mode 1; mode 2: 16 x
// v_mfma_f32_16x16x32_bf16, the same FLOPs) or
// the same number of v_fma_f32 (mode 0) and reports shader-clock cycles (s_memtime) and 100 MHz wall ticks (s_memrealtime):
// the frequency the chip actually sustains under a matrix-core load, i.e. what "fraction of the 2.4 GHz peak" can mean.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clock_probe_kernel(int iters, int mode, long* out) {
  typedef __attribute__((ext_vector_type(8))) __bf16 bf8;
  f32x16 acc[8];
  for (int i = 0; i < 8; ++i) for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  bf8 av, bv;
  for (int i = 0; i < 8; ++i) {                           // pseudo-random operands in [-1, 1): zero / constant data reads a higher clock
    uint32_t h = (threadIdx.x * 8u + i + blockIdx.x * 2048u) * 2654435761u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    av[i] = (__bf16)((float)(int)(h & 0xFFFF) * (1.f / 32768.f) - 1.f);
    bv[i] = (__bf16)((float)(int)(h >> 16) * (1.f / 32768.f) - 1.f);
  }
  float f = threadIdx.x * 1e-3f;
  const long c0 = __builtin_readcyclecounter();
  const long t0 = wall_clock64();
  if (mode == 1) {
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[i], 0, 0, 0);
    }
  } else if (mode == 2) {                                 // the same FLOPs per iteration as mode 1 on the 16x16x32 shape
    f32x4 a4[16];
    for (int i = 0; i < 16; ++i) for (int r = 0; r < 4; ++r) a4[i][r] = 0.f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int i = 0; i < 16; ++i) a4[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, a4[i], 0, 0, 0);
    }
    for (int i = 0; i < 16; ++i) f += a4[i][0];
  } else {
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int i = 0; i < 64; ++i) f = fmaf(f, 1.0001f, 0.5f);
    }
  }
  const long c1 = __builtin_readcyclecounter();
  const long t1 = wall_clock64();
  float sum = f;
  for (int i = 0; i < 8; ++i) sum += acc[i][0];
  if (threadIdx.x == 0) { out[2 * blockIdx.x] = c1 - c0; out[2 * blockIdx.x + 1] = t1 - t0; }
  if (sum == 123.456f) out[0] = 0;
}

extern "C" int osuf_clock_probe(int blocks, int iters, int mode, long* out, hipStream_t stream) {
  if (blocks <= 0 || iters <= 0 || !out) return OSUF_EINVAL;
  hipLaunchKernelGGL(clock_probe_kernel, dim3(blocks), dim3(256), 0, stream, iters, mode, out);
  return osuf_launch_status();
}

extern "C" int osuf_version(void) { return 1; }
