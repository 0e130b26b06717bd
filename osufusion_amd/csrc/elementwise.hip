// Layout conversion, the masked MSE, the optimizer, weight packing with LoRA / DoRA, and a clock probe (HBM-bound, 16 B per lane), gfx950.
// The sampling kernels (schedules, steps, inpainting, windows) are in sampling.hip.
#include "common.hpp"

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
struct AdamWArgs { float lr, beta1, beta2, eps, wd, inv_bc1, inv_sqrt_bc2; };

// The update of ONE element, written once: adamw_kernel and adamw_ema_kernel (vector body and scalar tail of both) call it.  Every fused
// multiply-add is spelled out and contraction is off for the rest: left to the compiler, the same source line became an fma in one kernel and
// a multiply plus an add in another (it did, between the four-wide body and the scalar tail), and the kernels' bits drifted apart.  The
// forms are the ones the four-wide body has always compiled to.
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, float gs, const AdamWArgs& a) {
#pragma clang fp contract(off)
  const float ge = g * gs;
  m = fmaf(1.f - a.beta1, ge, a.beta1 * m);
  v = fmaf(a.beta2, v, ((1.f - a.beta2) * ge) * ge);
  const float denom = fmaf(sqrtf(v), a.inv_sqrt_bc2, a.eps);
  p = fmaf(fmaf(-a.lr, a.wd, 1.f), p, -((a.lr * a.inv_bc1) * m / denom));
}

// ---- EMA tracks of the weights: e <- e + d (p - e), up to four tracks per pass -----------------------------------------------
// Track j is ema + j * ld (n floats).  d[j] = 1 - beta_j.  Two values are selects, not arithmetic: d == 0 neither reads nor writes the
// track, d >= 1 stores p without reading the track.  In between, one subtraction and one fused multiply-add (two roundings).
struct EmaArgs { float* ema; long ld; float d[4]; };

__device__ __forceinline__ bool ema_blends(float d) { return d > 0.f && d < 1.f; }
__device__ __forceinline__ float ema_element(float e, float p, float d) { return fmaf(d, p - e, e); }
__device__ __forceinline__ f32x4 ema_element(f32x4 e, f32x4 p, float d) {
#pragma unroll
  for (int c = 0; c < 4; ++c) e[c] = ema_element(e[c], p[c], d);
  return e;
}
// V = f32x4 (i counts vectors) or float (i counts elements).  The loads are a step of their own so that the fused kernel issues them
// ahead of the AdamW arithmetic; a track that does not blend loads nothing.
template <int TRACKS, typename V>
__device__ __forceinline__ void ema_load(const EmaArgs& a, long i, V (&e)[TRACKS]) {
#pragma unroll
  for (int j = 0; j < TRACKS; ++j)
    if (ema_blends(a.d[j])) e[j] = reinterpret_cast<const V*>(a.ema + j * a.ld)[i];
}
template <int TRACKS, typename V>
__device__ __forceinline__ void ema_store(const EmaArgs& a, long i, const V (&e)[TRACKS], V p) {
#pragma unroll
  for (int j = 0; j < TRACKS; ++j) {
    V* dst = reinterpret_cast<V*>(a.ema + j * a.ld) + i;
    if (ema_blends(a.d[j])) *dst = ema_element(e[j], p, a.d[j]);
    else if (a.d[j] >= 1.f) *dst = p;
  }
}

// TRACKS = 0 is torch.optim.AdamW alone (osuf_adamw); TRACKS = 1..4 also moves that many EMA tracks towards the parameter just written.
template <int TRACKS>
__device__ __forceinline__ void adamw_body(float* p, const float* g, float* m, float* v, long n, const AdamWArgs& a, const float* gscale,
                                           const EmaArgs& ea) {
  const float gs = gscale ? *gscale : 1.f;
  const long n4 = n >> 2;
  GRID_STRIDE(i, n4) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i], gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
    f32x4 ev[TRACKS ? TRACKS : 1];
    if constexpr (TRACKS > 0) ema_load<TRACKS>(ea, i, ev);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = pv[e], me = mv[e], ve = vv[e];
      adamw_element(pe, gv[e], me, ve, gs, a);
      pv[e] = pe; mv[e] = me; vv[e] = ve;
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    if constexpr (TRACKS > 0) ema_store<TRACKS>(ea, i, ev, pv);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    float pe = p[i], me = m[i], ve = v[i];
    float es[TRACKS ? TRACKS : 1];
    if constexpr (TRACKS > 0) ema_load<TRACKS>(ea, i, es);
    adamw_element(pe, g[i], me, ve, gs, a);
    p[i] = pe; m[i] = me; v[i] = ve;
    if constexpr (TRACKS > 0) ema_store<TRACKS>(ea, i, es, pe);
  }
}

__global__ __launch_bounds__(256) void adamw_kernel(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                                                    float eps, float wd, float inv_bc1, float inv_sqrt_bc2, const float* gscale) {
  adamw_body<0>(p, g, m, v, n, AdamWArgs{lr, beta1, beta2, eps, wd, inv_bc1, inv_sqrt_bc2}, gscale, EmaArgs{});
}

template <int TRACKS>
__global__ __launch_bounds__(256) void adamw_ema_kernel(float* p, const float* g, float* m, float* v, long n, AdamWArgs a, const float* gscale,
                                                        EmaArgs ea) {
  adamw_body<TRACKS>(p, g, m, v, n, a, gscale, ea);
}

// the tracks alone, from the parameters as they stand
template <int TRACKS>
__global__ __launch_bounds__(256) void ema_update_kernel(const float* p, long n, EmaArgs ea) {
  const long n4 = n >> 2;
  GRID_STRIDE(i, n4) {
    f32x4 ev[TRACKS];
    ema_load<TRACKS>(ea, i, ev);
    ema_store<TRACKS>(ea, i, ev, reinterpret_cast<const f32x4*>(p)[i]);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    float es[TRACKS];
    ema_load<TRACKS>(ea, i, es);
    ema_store<TRACKS>(ea, i, es, p[i]);
  }
}

// a <-> b, in place
__global__ __launch_bounds__(256) void swap_kernel(float* a, float* b, long n) {
  const long n4 = n >> 2;
  GRID_STRIDE(i, n4) {
    const f32x4 av = reinterpret_cast<f32x4*>(a)[i], bv = reinterpret_cast<f32x4*>(b)[i];
    reinterpret_cast<f32x4*>(a)[i] = bv;
    reinterpret_cast<f32x4*>(b)[i] = av;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    const float ae = a[i], be = b[i];
    a[i] = be; b[i] = ae;
  }
}

// ---- linear combination of up to eight fp32 buffers in an fp64 accumulator (post-hoc EMA: osufusion_amd/posthoc_ema.py) ----------------
// a = CONT ? acc[i] : 0;  a = fma(w[k], (double)src[k][i], a) for k = 0..K-1 in that order;  acc[i] = a (if acc);  out[i] = (float)a (if
// out).  The chain is sequential in k and fp64 is stored exactly, so a list of sources cut into several launches (CONT on all but the
// first) gives the bits of one launch.  Pointers and weights travel by value; K is a template parameter so that every index into them is
// a constant and all K loads are issued before the first fma.  The host drops the sources whose weight is zero before the launch (K = 0
// is then possible: the accumulator alone), so a skipped source costs no branch here and is never read.
struct LincombArgs { const float* src[8]; double w[8]; };
typedef __attribute__((ext_vector_type(2))) double f64x2;

__device__ __forceinline__ double lincomb_step(double w, float x, double a) {
#pragma clang fp contract(off)
  return __builtin_fma(w, (double)x, a);
}

// VEC: four elements per lane (every pointer 16-byte aligned, acc 32-byte) and a scalar tail; otherwise one element per lane.
template <int K, bool VEC>
__global__ __launch_bounds__(256) void lincomb_kernel(LincombArgs a, double* acc, float* out, long n, int cont) {
  if constexpr (VEC) {
    const long n4 = n >> 2;
    GRID_STRIDE(i, n4) {
      f32x4 x[K ? K : 1];
#pragma unroll
      for (int k = 0; k < K; ++k) x[k] = reinterpret_cast<const f32x4*>(a.src[k])[i];
      f64x2 lo = {0.0, 0.0}, hi = {0.0, 0.0};
      if (cont) { lo = reinterpret_cast<const f64x2*>(acc)[2 * i]; hi = reinterpret_cast<const f64x2*>(acc)[2 * i + 1]; }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        lo[0] = lincomb_step(a.w[k], x[k][0], lo[0]);
        lo[1] = lincomb_step(a.w[k], x[k][1], lo[1]);
        hi[0] = lincomb_step(a.w[k], x[k][2], hi[0]);
        hi[1] = lincomb_step(a.w[k], x[k][3], hi[1]);
      }
      if (acc) { reinterpret_cast<f64x2*>(acc)[2 * i] = lo; reinterpret_cast<f64x2*>(acc)[2 * i + 1] = hi; }
      if (out) {
        f32x4 o; o[0] = (float)lo[0]; o[1] = (float)lo[1]; o[2] = (float)hi[0]; o[3] = (float)hi[1];
        reinterpret_cast<f32x4*>(out)[i] = o;
      }
    }
  }
  const long first = VEC ? (n >> 2) << 2 : 0;               // VEC: the n % 4 elements left over; else all of them
  GRID_STRIDE(j, n - first) {
    const long i = first + j;
    float x[K ? K : 1];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = a.src[k][i];
    double v = cont ? acc[i] : 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) v = lincomb_step(a.w[k], x[k], v);
    if (acc) acc[i] = v;
    if (out) out[i] = (float)v;
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
  if (!in || !out || B <= 0 || C <= 0 || L <= 0 || KT <= 0 || width % 8 || ld % 8 || width < C * KT || width > ld || !al16(out)) return OSUF_EINVAL;
  const long tot = (long)B * L * (width / 8);
  if (dtype == OSUF_DT_BF16) hipLaunchKernelGGL(ncl_to_rows_kernel<bf16_t>, dim3(ew_grid(tot)), dim3(256), 0, stream, in, (bf16_t*)out, ld, width, B, C, L, KT);
  else if (dtype == OSUF_DT_F32) hipLaunchKernelGGL(ncl_to_rows_kernel<float>, dim3(ew_grid(tot)), dim3(256), 0, stream, in, (float*)out, ld, width, B, C, L, KT);
  else return OSUF_EUNSUPPORTED;
  return osuf_launch_status();
}

extern "C" int osuf_rows_to_ncl(int dtype, const void* in, long ld, float* out, int B, int C, int L, hipStream_t stream) {
  if (!in || !out || B <= 0 || C <= 0 || L <= 0 || ld < C) return OSUF_EINVAL;
  const long tot = (long)B * C * L;
  if (dtype == OSUF_DT_BF16) hipLaunchKernelGGL(rows_to_ncl_kernel<bf16_t>, dim3(ew_grid(tot)), dim3(256), 0, stream, (const bf16_t*)in, ld, out, B, C, L);
  else if (dtype == OSUF_DT_F32) hipLaunchKernelGGL(rows_to_ncl_kernel<float>, dim3(ew_grid(tot)), dim3(256), 0, stream, (const float*)in, ld, out, B, C, L);
  else return OSUF_EUNSUPPORTED;
  return osuf_launch_status();
}

extern "C" int osuf_copy2d(int src_dtype, const void* src, long lds_, int dst_dtype, void* dst, long ldd, int M, int cols, hipStream_t stream) {
  if (!src || !dst || M <= 0 || cols <= 0 || cols % 8 || lds_ % 8 || ldd % 8 || !al16(src) || !al16(dst)) return OSUF_EINVAL;
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
  if (!a || !b || !dst || M <= 0 || cols <= 0 || cols % 8 || lda % 8 || ldb % 8 || ldd % 8 || !al16(a) || !al16(b) || !al16(dst)) return OSUF_EINVAL;
  const long tot = (long)M * (cols / 8);
  if (dtype == OSUF_DT_BF16) hipLaunchKernelGGL(add2d_kernel<bf16_t>, dim3(ew_grid(tot)), dim3(256), 0, stream, (const bf16_t*)a, lda, (const bf16_t*)b, ldb, (bf16_t*)dst, ldd, M, cols);
  else if (dtype == OSUF_DT_F32) hipLaunchKernelGGL(add2d_kernel<float>, dim3(ew_grid(tot)), dim3(256), 0, stream, (const float*)a, lda, (const float*)b, ldb, (float*)dst, ldd, M, cols);
  else return OSUF_EUNSUPPORTED;
  return osuf_launch_status();
}

extern "C" int osuf_mse(const float* pred, const float* target, const int* orig_len, float* grad, double* loss_sum, int B, int Dch, int L,
                        hipStream_t stream) {
  if (!pred || !target || !loss_sum || B <= 0 || Dch <= 0 || L <= 0) return OSUF_EINVAL;
  const long tot = (long)B * Dch * L;
  hipLaunchKernelGGL(mse_kernel<false>, dim3(ew_grid(tot)), dim3(256), 0, stream, pred, target, orig_len, nullptr, grad, loss_sum, Dch, L, tot);
  return osuf_launch_status();
}

extern "C" int osuf_mse_w(const float* pred, const float* target, const int* orig_len, const float* w, float* grad, double* loss_sum, int B,
                          int Dch, int L, hipStream_t stream) {
  if (!pred || !target || !loss_sum || B <= 0 || Dch <= 0 || L <= 0 || !w) return OSUF_EINVAL;
  const long tot = (long)B * Dch * L;
  hipLaunchKernelGGL(mse_kernel<true>, dim3(ew_grid(tot)), dim3(256), 0, stream, pred, target, orig_len, w, grad, loss_sum, Dch, L, tot);
  return osuf_launch_status();
}

extern "C" int osuf_sqnorm(const float* g, long n, double* out, hipStream_t stream) {
  if (!g || !out || n <= 0 || !al16(g)) return OSUF_EINVAL;
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

// tracks in 1..4, every d >= 0, ld >= n; on the four-wide path (n >= 4) the base and the track stride must keep every track 16-byte aligned
static bool ema_args(float* ema, long ld, long n, int tracks, float d0, float d1, float d2, float d3, EmaArgs* out) {
  *out = EmaArgs{ema, ld, {d0, d1, d2, d3}};
  if (!ema || tracks < 1 || tracks > 4 || ld < n) return false;
  if (n >= 4 && (!al16(ema) || (ld & 3))) return false;
  for (int j = 0; j < tracks; ++j)
    if (!(out->d[j] >= 0.f)) return false;
  return true;
}
#define DISPATCH_TRACKS(tracks, ...)                 \
  switch (tracks) {                                  \
    case 1: { constexpr int TRACKS = 1; __VA_ARGS__; } break; \
    case 2: { constexpr int TRACKS = 2; __VA_ARGS__; } break; \
    case 3: { constexpr int TRACKS = 3; __VA_ARGS__; } break; \
    default: { constexpr int TRACKS = 4; __VA_ARGS__; } break; \
  }

extern "C" int osuf_adamw_ema(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, float wd,
                              int step, const float* gscale, float* ema, long ema_ld, int tracks, float d0, float d1, float d2, float d3,
                              hipStream_t stream) {
  EmaArgs ea;
  if (n <= 0 || step <= 0 || !al16(p) || !al16(g) || !al16(m) || !al16(v) || !ema_args(ema, ema_ld, n, tracks, d0, d1, d2, d3, &ea))
    return OSUF_EINVAL;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const AdamWArgs a{lr, beta1, beta2, eps, wd, (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2))};
  DISPATCH_TRACKS(tracks, hipLaunchKernelGGL(adamw_ema_kernel<TRACKS>, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, stream, p, g, m, v, n, a, gscale, ea));
  return osuf_launch_status();
}

extern "C" int osuf_ema_update(const float* p, float* ema, long ema_ld, long n, int tracks, float d0, float d1, float d2, float d3,
                               hipStream_t stream) {
  EmaArgs ea;
  if (n <= 0 || !al16(p) || !ema_args(ema, ema_ld, n, tracks, d0, d1, d2, d3, &ea)) return OSUF_EINVAL;
  DISPATCH_TRACKS(tracks, hipLaunchKernelGGL(ema_update_kernel<TRACKS>, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, stream, p, n, ea));
  return osuf_launch_status();
}

extern "C" int osuf_swap(float* a, float* b, long n, hipStream_t stream) {
  if (n <= 0 || !a || !b || !al16(a) || !al16(b)) return OSUF_EINVAL;
  if (a == b || (a < b ? b - a : a - b) < n) return OSUF_EINVAL;       // the same or overlapping buffers
  hipLaunchKernelGGL(swap_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, stream, a, b, n);
  return osuf_launch_status();
}

template <int K>
static void lincomb_launch(const LincombArgs& a, double* acc, float* out, long n, int cont, bool vec, hipStream_t stream) {
  if (vec) hipLaunchKernelGGL((lincomb_kernel<K, true>), dim3(ew_grid(n / 4 + 1)), dim3(256), 0, stream, a, acc, out, n, cont);
  else hipLaunchKernelGGL((lincomb_kernel<K, false>), dim3(ew_grid(n)), dim3(256), 0, stream, a, acc, out, n, cont);
}

// src and w are HOST arrays.  flags & 1: continue from acc.
extern "C" int osuf_lincomb(const float* const* src, const double* w, int K, double* acc, float* out, long n, int flags,
                            hipStream_t stream) {
  const int cont = flags & 1;
  if (!src || !w || K < 1 || K > 8 || n < 0 || (!acc && !out) || (cont && !acc)) return OSUF_EINVAL;
  LincombArgs a{};
  int used = 0;
  bool vec = (reinterpret_cast<uintptr_t>(acc) & 31) == 0 && al16(out);
  for (int k = 0; k < K; ++k) {
    if (w[k] != w[k]) return OSUF_EINVAL;
    if (w[k] == 0.0) continue;                             // a select: the source is neither read nor required to exist
    if (!src[k]) return OSUF_EINVAL;
    vec = vec && al16(src[k]);
    a.src[used] = src[k];
    a.w[used++] = w[k];
  }
  if (n == 0) return OSUF_OK;
  switch (used) {
    case 0: lincomb_launch<0>(a, acc, out, n, cont, vec, stream); break;
    case 1: lincomb_launch<1>(a, acc, out, n, cont, vec, stream); break;
    case 2: lincomb_launch<2>(a, acc, out, n, cont, vec, stream); break;
    case 3: lincomb_launch<3>(a, acc, out, n, cont, vec, stream); break;
    case 4: lincomb_launch<4>(a, acc, out, n, cont, vec, stream); break;
    case 5: lincomb_launch<5>(a, acc, out, n, cont, vec, stream); break;
    case 6: lincomb_launch<6>(a, acc, out, n, cont, vec, stream); break;
    case 7: lincomb_launch<7>(a, acc, out, n, cont, vec, stream); break;
    default: lincomb_launch<8>(a, acc, out, n, cont, vec, stream); break;
  }
  return osuf_launch_status();
}

extern "C" int osuf_clip_coef(const double* sumsq, float max_norm, float base, float* coef, float* total_norm, hipStream_t stream) {
  if (!sumsq || !coef) return OSUF_EINVAL;
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
  long n = (long)O * r;                                     // >= O, the third index range
  if ((long)r * I * k > n) n = (long)r * I * k;
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

// the override table of common.hpp: OSUF_KNOB_DEFAULT (-1) or a value >= 0; anything else, and an unknown slot, is refused
extern "C" int osuf_override_set(int knob, int value) {
  if (knob < 0 || knob >= OSUF_KNOB_COUNT || value < OSUF_KNOB_DEFAULT) return OSUF_EINVAL;
  osuf_knobs[knob].store(value, std::memory_order_relaxed);
  return OSUF_OK;
}
extern "C" int osuf_override_get(int knob, int* value) {
  if (knob < 0 || knob >= OSUF_KNOB_COUNT || !value) return OSUF_EINVAL;
  *value = osuf_knob(knob);
  return OSUF_OK;
}
