// DiT row kernels (osu_fusion/modules/dit.py): adaLN-Zero modulation, per-head QK RMS-norm, audio statistics pooling.
//
// Rows are [M][C] with M = B * L; the sample of row m is m / L.  One wave per row, lane i owning the 8-element chunks i, i + 64, ...
// (16-B loads for bf16, 2 x 16 B for fp32).  Reductions across rows never use atomics: every workgroup stores its partial sums and a
// second kernel adds them in workgroup order, so the results are bit-identical from launch to launch.
#include "common.hpp"

static inline int chunk_iters(int chunks) { const int j = (chunks + 63) / 64; return j <= 1 ? 1 : j <= 2 ? 2 : j <= 4 ? 4 : j <= 8 ? 8 : 0; }

// ------------------------------------------------------------------------------------------------
// adaLN:  out = LN(x) * (1 + scale[b]) + shift[b]    (LayerNorm without affine, dit.py:14-15,135,143,76)
// ------------------------------------------------------------------------------------------------
template <typename T, int J>
__global__ __launch_bounds__(256) void adaln_fwd_kernel(const T* x, long ldx, T* out, long ldo, float* mr, const float* shift,
                                                        const float* scale, long ldm, int M, int C, int L, float eps) {
  const int chunks = C >> 3;
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long waves = ((long)gridDim.x * blockDim.x) >> 6;
  const float invC = 1.f / (float)C;
  for (long m = wave; m < M; m += waves) {
    float v[J][8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int ch = lane + 64 * j;
      if (ch < chunks) {
        load8(x + m * ldx + ch * 8, v[j]);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[j][e];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[j][e] = 0.f;
      }
    }
    const float mean = group_sum<64>(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      if (lane + 64 * j < chunks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[j][e] - mean; q += d * d; }
      }
    }
    const float rstd = rsqrtf(group_sum<64>(q) * invC + eps);
    if (lane == 0 && mr) { mr[2 * m] = mean; mr[2 * m + 1] = rstd; }
    const long b = m / L;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int ch = lane + 64 * j;
      if (ch < chunks) {
        float sh[8], sc[8], o[8];
        load8(shift + b * ldm + ch * 8, sh);
        load8(scale + b * ldm + ch * 8, sc);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v[j][e] - mean) * rstd * (1.f + sc[e]) + sh[e];
        store8(out + m * ldo + ch * 8, o);
      }
    }
  }
}

// grid (nblk, B): workgroup k of sample b takes the rows n = 4 k + wave, stepping by 4 nblk, of that sample.
// dx = dres + rstd * (g - mean_c g - xhat * mean_c(g * xhat)),  g = dy * (1 + scale[b]);
// partial[b][k][0][c] = sum dy,  partial[b][k][1][c] = sum dy * xhat over the workgroup's rows
template <typename T, int J>
__global__ __launch_bounds__(256) void adaln_bwd_kernel(const T* dy, long lddy, const T* x, long ldx, const T* dres, long ldr, T* dx, long lddx,
                                                        const float* mr, const float* scale, long ldm, float* part, int C, int L) {
  const int chunks = C >> 3;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.y, k = blockIdx.x, nblk = gridDim.x;
  const float invC = 1.f / (float)C;
  float sc[J][8], ash[J][8], asc[J][8];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int ch = lane + 64 * j;
    if (ch < chunks) load8(scale + (long)b * ldm + ch * 8, sc[j]);
#pragma unroll
    for (int e = 0; e < 8; ++e) { ash[j][e] = 0.f; asc[j][e] = 0.f; if (ch >= chunks) sc[j][e] = 0.f; }
  }
  for (long n = 4L * k + wv; n < L; n += 4L * nblk) {
    const long m = (long)b * L + n;
    const float mean = mr[2 * m], rstd = mr[2 * m + 1];
    float xh[J][8], g[J][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int ch = lane + 64 * j;
      if (ch < chunks) {
        float xv[8], dv[8];
        load8(x + m * ldx + ch * 8, xv);
        load8(dy + m * lddy + ch * 8, dv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xh[j][e] = (xv[e] - mean) * rstd;
          g[j][e] = dv[e] * (1.f + sc[j][e]);
          s1 += g[j][e];
          s2 += g[j][e] * xh[j][e];
          ash[j][e] += dv[e];
          asc[j][e] += dv[e] * xh[j][e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { xh[j][e] = 0.f; g[j][e] = 0.f; }
      }
    }
    s1 = group_sum<64>(s1) * invC;
    s2 = group_sum<64>(s2) * invC;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int ch = lane + 64 * j;
      if (ch < chunks) {
        float o[8], r[8];
        if (dres) load8(dres + m * ldr + ch * 8, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = rstd * (g[j][e] - s1 - xh[j][e] * s2) + (dres ? r[e] : 0.f);
        store8(dx + m * lddx + ch * 8, o);
      }
    }
  }
  // the four waves' sums meet in LDS and are added in wave order
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem);                 // [4][2][C]
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int ch = lane + 64 * j;
    if (ch < chunks) {
      store8(red + (wv * 2 + 0) * C + ch * 8, ash[j]);
      store8(red + (wv * 2 + 1) * C + ch * 8, asc[j]);
    }
  }
  __syncthreads();
  float* dst = part + ((long)b * nblk + k) * 2 * C;
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) dst[i] = red[i] + red[2 * C + i] + red[4 * C + i] + red[6 * C + i];
}

// out[b][c] (row stride ldo; columns 0..C-1 dshift, then at out + off2 the C dscale columns) = sum over k of part[b][k][.][c].
// A 64 x 16 workgroup per 64 columns: slice y adds k = y, y + 16, ... in order, then the 16 slice sums are added in slice order (fixed).
static constexpr int kFinCols = 64, kFinSlices = 16;
__global__ __launch_bounds__(kFinCols * kFinSlices) void rowpart_finish_kernel(const float* part, int nblk, int W, float* out, long ldo, long off2, int C) {
  __shared__ float red[kFinSlices][kFinCols];
  const int b = blockIdx.y, tx = threadIdx.x % kFinCols, ty = threadIdx.x / kFinCols;
  const int i = blockIdx.x * kFinCols + tx;
  float s = 0.f;
  if (i < W) {
    const float* p = part + (long)b * nblk * W + i;
#pragma unroll 8
    for (int k = ty; k < nblk; k += kFinSlices) s += p[(long)k * W];
  }
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && i < W) {
    float t = 0.f;
#pragma unroll
    for (int y = 0; y < kFinSlices; ++y) t += red[y][tx];
    const int half = i / C, c = i - half * C;
    out[(long)b * ldo + (half ? off2 : 0) + c] = t;
  }
}

static int adaln_bwd_blocks(int B, int L) {
  int nblk = (L + 15) / 16;                                   // >= 4 rows per wave
  const int cap = 2048 / B > 1 ? 2048 / B : 1;                // ~2,048 workgroups over the batch
  return nblk < cap ? nblk : cap;
}

extern "C" int osuf_adaln_fwd(int dtype, const void* x, long ldx, void* out, long ldo, float* mr, const float* shift, const float* scale, long ldm,
                              int M, int C, int L, float eps, hipStream_t stream) {
  if (bad_c(C) || M <= 0 || L <= 0 || M % L || ldx % 8 || ldo % 8 || ldm % 4 || !al16(x) || !al16(out) || !al16(shift) || !al16(scale))
    return OSUF_EINVAL;
  if (!x || !out || !shift || !scale || ldx < C || ldo < C || ldm < C) return OSUF_EINVAL;       // mr may be NULL: mean and rstd are then not kept
  const int J = chunk_iters(C / 8);
  long blocks = ((long)M + 3) / 4;
  if (blocks > 4096) blocks = 4096;
#define ADALN_FWD(J_) hipLaunchKernelGGL((adaln_fwd_kernel<T, J_>), dim3((int)blocks), dim3(256), 0, stream, (const T*)x, ldx, (T*)out, ldo, mr, shift, scale, ldm, M, C, L, eps)
  DISPATCH_T(dtype, if (J == 1) ADALN_FWD(1); else if (J == 2) ADALN_FWD(2); else ADALN_FWD(4));
#undef ADALN_FWD
  return osuf_launch_status();
}

extern "C" long osuf_adaln_bwd_workspace_bytes(int M, int C, int L) {
  if (bad_c(C) || M <= 0 || L <= 0 || M % L || M / L > 65535) return 0;
  const int B = M / L;
  return (long)B * adaln_bwd_blocks(B, L) * 2 * C * (long)sizeof(float);
}

/* dx = dres + LN-backward(dy * (1 + scale[b])); dshift[b][c] = sum_n dy, dscale[b][c] = sum_n dy * xhat, stored (not added) at
 * dmod[b * ldd + c] and dmod[b * ldd + off2 + c].  dres may be NULL.  workspace: osuf_adaln_bwd_workspace_bytes(M, C, L) bytes. */
extern "C" int osuf_adaln_bwd(int dtype, const void* dy, long lddy, const void* x, long ldx, const void* dres, long ldr, void* dx, long lddx,
                              const float* mr, const float* scale, long ldm, float* dmod, long ldd, long off2, float* workspace,
                              long workspace_bytes, int M, int C, int L, hipStream_t stream) {
  if (bad_c(C) || M <= 0 || L <= 0 || M % L || M / L > 65535 || lddy % 8 || ldx % 8 || lddx % 8 || (dres && ldr % 8) || ldm % 4 || !mr || !dmod || !workspace)
    return OSUF_EINVAL;
  if (!al16(dy) || !al16(x) || !al16(dx) || (dres && !al16(dres)) || !al16(scale)) return OSUF_EINVAL;
  if (!dy || !x || !dx || !scale || lddy < C || ldx < C || lddx < C || (dres && ldr < C) || ldm < C || ldd < C) return OSUF_EINVAL;
  if (workspace_bytes < osuf_adaln_bwd_workspace_bytes(M, C, L)) return OSUF_EINVAL;
  const int B = M / L, J = chunk_iters(C / 8), nblk = adaln_bwd_blocks(B, L);
  const size_t lds = (size_t)8 * C * sizeof(float);
#define ADALN_BWD(J_) hipLaunchKernelGGL((adaln_bwd_kernel<T, J_>), dim3(nblk, B), dim3(256), lds, stream, (const T*)dy, lddy, (const T*)x, ldx, \
                                         (const T*)dres, ldr, (T*)dx, lddx, mr, scale, ldm, workspace, C, L)
  DISPATCH_T(dtype, if (J == 1) ADALN_BWD(1); else if (J == 2) ADALN_BWD(2); else ADALN_BWD(4));
#undef ADALN_BWD
  hipLaunchKernelGGL(rowpart_finish_kernel, dim3((2 * C + kFinCols - 1) / kFinCols, B), dim3(kFinCols * kFinSlices), 0, stream, workspace, nblk, 2 * C,
                     dmod, ldd, off2, C);
  return osuf_launch_status();
}

// ------------------------------------------------------------------------------------------------
// QK RMS-norm of raw q|k|v projection rows [M][(H + 2G) D] = [q (h d) | k (g d) | v (g d)]   (dit.py:63-70,109-113, mmdit.py:94-127)
//   y = x / max(||x||, 1e-12) * gamma[h] * sqrt(D) for the q and k heads, v copied; one bf16 rounding (what Attend reads)
// A head is D / 8 consecutive lanes (16 B each): its sum of squares is a butterfly over those lanes.
// The normed rows land in joint attention rows: two streams' projections packed into one bf16 buffer over [audio; map].
//   rows:    sample b owns Nj joint rows; a stream with Ns rows per sample at row offset `off` puts its row m = b * Ns + n at b * Nj + off + n
//   columns: [H q heads GROUP-MAJOR | G k heads | G v heads], D each.  The reference repeats K/V as "b h n d -> b (r h) n d", so natural
//            query head j reads K/V head j % G: it goes to column block (j % G) * (H / G) + j / G (what ops.mqa_fwd(kv_heads=G) reads)
// One entry-point call serves ONE stream (an MMDiT layer calls each twice); the other stream's joint rows are never touched.  The DiT is
// the one-stream case Ns == Nj, off == 0, G == H: both maps are then the identity and the joint rows are the plain q|k|v rows.
// ------------------------------------------------------------------------------------------------
static constexpr float kNormEps = 1e-12f;
static int qknorm_bwd_blocks(int M) { long b = ((long)M + 15) / 16; return (int)(b < 1024 ? b : 1024); }

__device__ __forceinline__ long joint_row(long m, int Ns, int Nj, int off) {
  const long b = m / Ns;
  return b * Nj + off + (m - b * Ns);
}
// 8-element chunk `ch` of a stream's row (natural head order, hc chunks per head) -> its chunk in the joint row
__device__ __forceinline__ int joint_chunk(int ch, int hc, int H, int G) {
  const int head = ch / hc;
  if (head >= H) return ch;                                      // k and v heads keep their place
  return ((head % G) * (H / G) + head / G) * hc + (ch - head * hc);
}

// raw q|k|v rows [M][(H + 2G) D] (T) -> bf16 joint rows, the q and k heads normed; gq == NULL: cast only.  inv[m][H + G]: the stream's
// own rows, natural head order (q heads, then k heads).  JOINT false: one stream with G == H, where joint_row and joint_chunk are the
// identity; their 64-bit division per row and integer divisions per chunk cost this light kernel 7 % at the DiT's shape
// (profiles/qknorm_fold.md), so the launcher leaves them out at compile time.  The backward does enough arithmetic to hide them.
template <typename T, int J, bool JOINT>
__global__ __launch_bounds__(256) void joint_qknorm_fwd_kernel(const T* x, long ldx, bf16_t* y, long ldy, float* inv, const float* gq, const float* gk,
                                                               int M, int Ns, int Nj, int off, int H, int G, int D) {
  const int hc = D / 8, chunks = (H + 2 * G) * hc, qk = (H + G) * hc;
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long waves = ((long)gridDim.x * blockDim.x) >> 6;
  const float sD = sqrtf((float)D);
  for (long m = wave; m < M; m += waves) {
    const long jr = JOINT ? joint_row(m, Ns, Nj, off) : m;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int ch = lane + 64 * j;
      if (ch >= chunks) break;                                  // whole heads drop out together (64 and chunks are multiples of D / 8)
      float v[8];
      load8(x + m * ldx + ch * 8, v);
      if (gq && ch < qk) {
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) q += v[e] * v[e];
        q = group_sum_dyn(q, hc);
        const float r = 1.f / fmaxf(sqrtf(q), kNormEps);
        const int head = ch / hc;                               // 0 .. H + G - 1: q heads, then k heads
        const float* g = (head < H ? gq + head * D : gk + (head - H) * D) + (ch % hc) * 8;
        float gv[8];
        load8(g, gv);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] * r * gv[e] * sD;
        if (ch % hc == 0) inv[m * (H + G) + head] = r;
      }
      store8(y + jr * ldy + (JOINT ? joint_chunk(ch, hc, H, G) : ch) * 8, v);
    }
  }
}

// PACK: a stream's rows [M][H D] (T, natural head order) -> its bf16 joint rows (group-major); else the way back.
template <typename T, bool PACK>
__global__ __launch_bounds__(256) void joint_perm_kernel(T* s, long lds, bf16_t* joint, long ldj, int M, int Ns, int Nj, int off, int H, int G, int D) {
  const int hc = D / 8, chunks = H * hc;
  const long total = (long)M * chunks;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / chunks;
    const int ch = (int)(i - m * chunks);
    T* ps = s + m * lds + ch * 8;
    bf16_t* pj = joint + joint_row(m, Ns, Nj, off) * ldj + joint_chunk(ch, hc, H, G) * 8;
    float v[8];
    if (PACK) { load8(ps, v); store8(pj, v); }
    else { load8(pj, v); store8(ps, v); }
  }
}

// fp32 dq|dk|dv JOINT rows (ops.mqa_bwd) -> gradient of one stream's raw projections (T, natural head order).  Per q / k head, with
// u = x / max(n, eps), gu = g gamma sqrt(D):
//   n >= eps: dx = (gu - u (u . gu)) / n;   n < eps (the clamp holds the norm constant): dx = gu / eps.
// dgamma partials (gq != NULL only): part[k][(H + G) D] = sum over the workgroup's rows of g * u * sqrt(D).
template <typename T, int J>
__global__ __launch_bounds__(256) void joint_qknorm_bwd_kernel(const float* g, long ldg, const T* x, long ldx, const float* inv, const float* gq,
                                                               const float* gk, T* dx, long lddx, float* part, int M, int Ns, int Nj, int off,
                                                               int H, int G, int D) {
  const int hc = D / 8, chunks = (H + 2 * G) * hc, qk = (H + G) * hc;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float sD = sqrtf((float)D);
  float acc[J][8];
#pragma unroll
  for (int j = 0; j < J; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
  for (long m = 4L * blockIdx.x + wv; m < M; m += 4L * gridDim.x) {
    const long jr = joint_row(m, Ns, Nj, off);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int ch = lane + 64 * j;
      if (ch >= chunks) break;
      float gv[8];
      load8(g + jr * ldg + joint_chunk(ch, hc, H, G) * 8, gv);
      if (gq && ch < qk) {
        float xv[8], ga[8];
        load8(x + m * ldx + ch * 8, xv);
        const int head = ch / hc;
        load8((head < H ? gq + head * D : gk + (head - H) * D) + (ch % hc) * 8, ga);
        const float r = inv[m * (H + G) + head];
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) q += xv[e] * xv[e];
        q = group_sum_dyn(q, hc);
        const bool clamped = sqrtf(q) < kNormEps;
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float u = xv[e] * r;
          acc[j][e] += gv[e] * u * sD;
          gv[e] *= ga[e] * sD;                                  // gu
          xv[e] = u;
          d += u * gv[e];
        }
        d = group_sum_dyn(d, hc);
        if (clamped) d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) gv[e] = (gv[e] - xv[e] * d) * r;
      }
      store8(dx + m * lddx + ch * 8, gv);
    }
  }
  if (!gq) return;                                               // (uniform: no workgroup meets the barrier half way)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem);                 // [4][(H + G) D]
  const int W = (H + G) * D;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int ch = lane + 64 * j;
    if (ch < qk) store8(red + wv * W + ch * 8, acc[j]);
  }
  __syncthreads();
  float* dst = part + (long)blockIdx.x * W;
  for (int i = threadIdx.x; i < W; i += blockDim.x) dst[i] = red[i] + red[W + i] + red[2 * W + i] + red[3 * W + i];
}

static bool bad_joint(int M, int Ns, int Nj, int off, int H, int G, int D) {
  return M <= 0 || Ns <= 0 || Nj <= 0 || off < 0 || (long)off + Ns > Nj || M % Ns || H <= 0 || G <= 0 || H % G ||
         !(D == 16 || D == 32 || D == 64 || D == 128) || ((long)H + 2L * G) * D > 4096;
}

extern "C" int osuf_joint_qknorm_fwd(int dtype, const void* x, long ldx, void* y, long ldy, float* inv, const float* gamma_q, const float* gamma_k,
                                     int M, int Ns, int Nj, int off, int H, int G, int D, hipStream_t stream) {
  if (bad_joint(M, Ns, Nj, off, H, G, D) || ldx % 8 || ldy % 8 || ldx < (long)(H + 2 * G) * D || ldy < (long)(H + 2 * G) * D || !al16(x) || !x || !y || !al16(y))
    return OSUF_EINVAL;
  if ((gamma_q == nullptr) != (gamma_k == nullptr) || (gamma_q && !inv) || !al16(gamma_q) || !al16(gamma_k)) return OSUF_EINVAL;
  const int J = chunk_iters((H + 2 * G) * D / 8);
  if (J == 0) return OSUF_EUNSUPPORTED;
  long blocks = ((long)M + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  const bool joint = !(Ns == Nj && off == 0 && G == H);       // else one stream, identity permutation (the DiT)
#define JQKN_FWD(J_, JOINT_) hipLaunchKernelGGL((joint_qknorm_fwd_kernel<T, J_, JOINT_>), dim3((int)blocks), dim3(256), 0, stream, (const T*)x, ldx, \
                                                (bf16_t*)y, ldy, inv, gamma_q, gamma_k, M, Ns, Nj, off, H, G, D)
#define JQKN_FWD_J(JOINT_) if (J == 1) JQKN_FWD(1, JOINT_); else if (J == 2) JQKN_FWD(2, JOINT_); else if (J == 4) JQKN_FWD(4, JOINT_); else JQKN_FWD(8, JOINT_)
  DISPATCH_T(dtype, if (joint) { JQKN_FWD_J(true); } else { JQKN_FWD_J(false); });
#undef JQKN_FWD_J
#undef JQKN_FWD
  return osuf_launch_status();
}

static int joint_perm(bool pack, int dtype, void* s, long lds, void* joint, long ldj, int M, int Ns, int Nj, int off, int H, int G, int D,
                      hipStream_t stream) {
  if (bad_joint(M, Ns, Nj, off, H, G, D) || lds % 8 || ldj % 8 || lds < (long)H * D || ldj < (long)H * D || !s || !joint || !al16(s) || !al16(joint))
    return OSUF_EINVAL;
  const int grid = ew_grid((long)M * (H * D / 8));
#define JPERM(P_) hipLaunchKernelGGL((joint_perm_kernel<T, P_>), dim3(grid), dim3(256), 0, stream, (T*)s, lds, (bf16_t*)joint, ldj, M, Ns, Nj, off, H, G, D)
  DISPATCH_T(dtype, if (pack) JPERM(true); else JPERM(false));
#undef JPERM
  return osuf_launch_status();
}

extern "C" int osuf_joint_pack(int dtype, const void* x, long ldx, void* joint, long ldj, int M, int Ns, int Nj, int off, int H, int G, int D,
                               hipStream_t stream) {
  return joint_perm(true, dtype, const_cast<void*>(x), ldx, joint, ldj, M, Ns, Nj, off, H, G, D, stream);
}

extern "C" int osuf_joint_unpack(int dtype, const void* joint, long ldj, void* out, long ldo, int M, int Ns, int Nj, int off, int H, int G, int D,
                                 hipStream_t stream) {
  return joint_perm(false, dtype, out, ldo, const_cast<void*>(joint), ldj, M, Ns, Nj, off, H, G, D, stream);
}

extern "C" long osuf_joint_qknorm_bwd_workspace_bytes(int M, int H, int G, int D) {
  if (bad_joint(M, 1, 1, 0, H, G, D)) return 0;
  return (long)qknorm_bwd_blocks(M) * (H + G) * D * (long)sizeof(float);
}

/* g: fp32 dq|dk|dv joint rows; x: the stream's raw projections (T), inv: the forward's [M][H + G].  dx in T, natural head order.  With
 * gammas, dgamma = [dgamma_q [H][D] | dgamma_k [G][D]] fp32 is stored (not added), summed in a fixed order through `workspace`
 * (osuf_joint_qknorm_bwd_workspace_bytes bytes); without (both NULL) the kernel only permutes and casts: inv, dgamma and workspace unused. */
extern "C" int osuf_joint_qknorm_bwd(int dtype, const float* g, long ldg, const void* x, long ldx, const float* inv, const float* gamma_q,
                                     const float* gamma_k, void* dx, long lddx, float* dgamma, float* workspace, long workspace_bytes,
                                     int M, int Ns, int Nj, int off, int H, int G, int D, hipStream_t stream) {
  if (bad_joint(M, Ns, Nj, off, H, G, D) || ldg % 4 || ldx % 8 || lddx % 8 || ldg < (long)(H + 2 * G) * D || lddx < (long)(H + 2 * G) * D || !g || !dx ||
      !al16(g) || !al16(dx))
    return OSUF_EINVAL;
  if ((gamma_q == nullptr) != (gamma_k == nullptr) || !al16(gamma_q) || !al16(gamma_k)) return OSUF_EINVAL;
  const bool norm = gamma_q != nullptr;
  if (norm && (!x || !al16(x) || ldx < (long)(H + 2 * G) * D || !inv || !dgamma || !workspace ||
               workspace_bytes < osuf_joint_qknorm_bwd_workspace_bytes(M, H, G, D)))
    return OSUF_EINVAL;
  const int J = chunk_iters((H + 2 * G) * D / 8), nblk = qknorm_bwd_blocks(M), W = (H + G) * D;
  if (J == 0) return OSUF_EUNSUPPORTED;
  const size_t lds = norm ? (size_t)4 * W * sizeof(float) : 0;
#define JQKN_BWD(J_) hipLaunchKernelGGL((joint_qknorm_bwd_kernel<T, J_>), dim3(nblk), dim3(256), lds, stream, g, ldg, (const T*)x, ldx, inv, gamma_q, gamma_k, \
                                        (T*)dx, lddx, workspace, M, Ns, Nj, off, H, G, D)
  DISPATCH_T(dtype, if (J == 1) JQKN_BWD(1); else if (J == 2) JQKN_BWD(2); else if (J == 4) JQKN_BWD(4); else JQKN_BWD(8));
#undef JQKN_BWD
  // one "sample" of (H + G) D columns: the first H D go to dgamma, the rest behind them (off2 = H D): [dgamma_q | dgamma_k]
  if (norm)
    hipLaunchKernelGGL(rowpart_finish_kernel, dim3((W + kFinCols - 1) / kFinCols, 1), dim3(kFinCols * kFinSlices), 0, stream, workspace, nblk, W, dgamma,
                       (long)0, (long)H * D, H * D);
  return osuf_launch_status();
}

// ------------------------------------------------------------------------------------------------
// audio statistics pooling (dit.py:275-277): out[b] = [mean_l a[b][c][l] | std_l a[b][c][l] (unbiased)], fp32 (B, C, L) contiguous
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stat_pool_kernel(const float* a, float* out, int C, int L) {
  const int b = blockIdx.y, c = blockIdx.x;
  const float* row = a + ((long)b * C + c) * L;
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float s = 0.f;
  for (int l = threadIdx.x; l < L; l += 256) s += row[l];
  s = group_sum<64>(s);
  if (lane == 0) red[wv] = s;
  __syncthreads();
  const float mean = (red[0] + red[1] + red[2] + red[3]) / (float)L;
  __syncthreads();
  float q = 0.f;
  for (int l = threadIdx.x; l < L; l += 256) { const float d = row[l] - mean; q += d * d; }
  q = group_sum<64>(q);
  if (lane == 0) red[wv] = q;
  __syncthreads();
  if (threadIdx.x == 0) {
    out[(long)b * 2 * C + c] = mean;
    out[(long)b * 2 * C + C + c] = sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)(L - 1));      // L = 1: 0 / 0 = NaN, as torch
  }
}

extern "C" int osuf_stat_pool(const float* a, float* out, int B, int C, int L, hipStream_t stream) {
  if (!a || !out || B <= 0 || C <= 0 || L <= 0 || B > 65535) return OSUF_EINVAL;
  hipLaunchKernelGGL(stat_pool_kernel, dim3(C, B), dim3(256), 0, stream, a, out, C, L);
  return osuf_launch_status();
}
