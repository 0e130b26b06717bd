/* osufusion_hip.h -- C ABI of libosuf_hip.so: the MI355X (gfx950) kernels behind the OsuFusion denoiser hot path.
 *
 * The reference (fauzanardh/OsuFusion) has no FFI/plugin layer: its boundary is the Python nn.Module API of
 * osu_fusion.modules.{unet,residual,attention} / osu_fusion.models.diffusion.  Every
 * entry point below replaces the vendor kernel(s) that one reference call site reaches through torch; the
 * citation after "replaces:" is that call site (paths relative to /root/reference/osu_fusion).
 *
 * Conventions
 *   - plain device pointers + sizes + hipStream_t; no allocation, no host sync, graph-capturable.  Nothing is kept between
 *     calls except two things: the one-time hipFuncSetAttribute registration of kernels that need > 64 KiB of LDS, and the
 *     per-process override table below (osuf_override_set).  Kernel variants are chosen per call (`variant` arguments); the
 *     table forces the few launcher branches that have no such argument, so that tests can compare one path bit for bit with
 *     another and A/B runs can time it.  It is a test and A/B aid, not configuration: every slot starts at its default, the
 *     launchers read it on every call, and nothing is read from the environment;
 *   - return 0 on success, <0 for an argument error (OSUF_EINVAL -1 invalid, OSUF_EUNSUPPORTED -2 unsupported), >0 = hipError_t of the launch;
 *   - activations are channels-last rows [B*L][C] ("rows"), C contiguous, row stride `ld*` in ELEMENTS;
 *   - dtype: 0 = fp32 storage (exact-f32 MFMA), 1 = bf16 storage (bf16 MFMA, fp32 accumulate);
 *   - all row strides / channel counts must be multiples of 8 elements, pointers 16-byte aligned.
 */
#ifndef OSUFUSION_HIP_H
#define OSUFUSION_HIP_H

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status of every `int` entry point: OSUF_OK, one of the two argument errors, or the (positive) hipError_t of the launch */
#define OSUF_OK 0
#define OSUF_EINVAL (-1)
#define OSUF_EUNSUPPORTED (-2)

#define OSUF_DT_F32 0
#define OSUF_DT_BF16 1
#define OSUF_DT_F32X3 2   /* osuf_gemm_nt / osuf_gemm_tn only: fp32 storage, every product as three bf16 MFMAs on split operands
                             (a = bf16(a) + bf16(a - bf16(a)): inputs kept to ~17 bits) -- 3/16 of the cost of the exact-f32 MFMA */
/* `variant` of the attention-backward entry points: AUTO picks by shape, PLAIN / PIPE force the plain or the software-pipelined kernel */
#define OSUF_ATTN_AUTO 0
#define OSUF_ATTN_PLAIN 1
#define OSUF_ATTN_PIPE 2
/* `dq_mode` of osuf_mqa_bwd_fused: fp32 atomics (default), or per-key-block slabs summed in a fixed order */
#define OSUF_DQ_ATOMIC 0          /* fp32 atomics; the sweep (256 or 512 keys per workgroup) is picked by shape */
#define OSUF_DQ_SLABS 1
#define OSUF_DQ_ATOMIC_256 2      /* force the 8-wave, 256-key sweep */
#define OSUF_DQ_ATOMIC_512 3      /* force the 4-wave, 512-key sweep (whole 512-key blocks: N % 512 == 0, else OSUF_EUNSUPPORTED) */
#define OSUF_DQ_ATOMIC_512A 5     /* the 512-key sweep with its hand-placed loop (tools/gen_attn_bwd512.py): dK / dV bit-identical to
                                     OSUF_DQ_ATOMIC_512; whole 512-key blocks and an even number of (head, query block) pairs per part */
#define OSUF_DQ_PREZEROED 0x100   /* flag, OR-ed into an atomic dq_mode: the dQ accumulator at the head of `workspace` was zero-filled by
                                     osuf_mqa_fwd_zdq of the same layer (the entry point then issues no memset) */
                                  /* (4 was a timing-only build of the 512-key sweep, since removed: refused with OSUF_EINVAL) */

int osuf_version(void);

/* ---- the override table (test and A/B aid) ---------------------------------------------------------------
 * One int per launcher branch that can be forced; OSUF_KNOB_DEFAULT in every slot at load.  The boolean slots are on for a value > 0. */
enum {
  OSUF_KNOB_GEMM_BIG_MIN_TILES,   /* osuf_gemm_nt / osuf_gemm_tn / osuf_gemm_tn_workspace_bytes: when the 256 x 256 kernels are picked.  Default: from
                                     192 tiles and N >= 192 on; 0: never; n > 0: from n tiles on, whatever N (1 forces them, the wgrad plan included) */
  OSUF_KNOB_GEMM_NO8P,            /* osuf_gemm_nt: the one-barrier-per-K-step 256 x 256 loops instead of the 8-phase ones */
  OSUF_KNOB_GEMM_NOHALO,          /* osuf_gemm_nt / osuf_gemm_tn: k = 3 convolutions on the plain kernels, not the shared-panel / merged-taps ones */
  OSUF_KNOB_WGRAD_F32_PARTIALS,   /* osuf_gemm_tn: fp32 partial tiles in the workspace instead of bf16 pairs */
  OSUF_KNOB_ATTN_FWD_NOWHOLE,     /* attention forward: the bounds-checked kernel also where N % 64 == 0 */
  OSUF_KNOB_ATTN_FWD_NOQSK,       /* attention forward on pre-scaled queries: osuf_mqa_fwd's kernel at a unit exponent scale, not their own */
  OSUF_KNOB_COUNT
};
#define OSUF_KNOB_DEFAULT (-1)
/* value: OSUF_KNOB_DEFAULT or >= 0.  An unknown knob or a value below OSUF_KNOB_DEFAULT is OSUF_EINVAL (-1) and changes nothing. */
int osuf_override_set(int knob, int value);
int osuf_override_get(int knob, int* value);

/* ---- conv1d / linear as tap-GEMMs (gemm.hip) -------------------------------------------------------------
 * C[m][n] = act( sum_t sum_k A[rowmap(m,t)][k] * W[t][n][k] + bias[n] ) * silu'(U[m][n]) + R[m][n] * rscale[b][n]
 * rowmap modes: 0 plain (stride/pad), 1 reflect-right (Downsample), 2 nearest-x2 input (Upsample), 3 dgrad of 1.
 * C2 (optional) receives the pre-activation; stats (optional, double [B][2]) accumulates per-sample sum / sum^2
 * of the stored output for the following GroupNorm(1, C).
 * replaces: nn.Conv1d in Block.proj (modules/residual.py:70,76), res_conv (residual.py:115,137),
 *           Downsample/Upsample/Parallel convs (modules/unet.py:66-69,81-87,95-101,219-236), CrossEmbedLayer
 *           (unet.py:42-58), final_conv (unet.py:354,513); nn.Linear to_q/to_kv/to_out (unet.py:118-123,129-141),
 *           FeedForward (unet.py:149-156), time/cond/FiLM MLPs (unet.py:356-366, residual.py:104-111,126-129),
 *           GlobalContext 1x1 MLP (residual.py:22-27); and autograd's input-gradient of each of them. */
int osuf_gemm_nt(int dtype, const void* A, long lda, const void* W, long ldw, long tapstride,
                 void* C, long ldc, void* C2, long ldc2, const void* R, long ldr, const void* U, long ldu,
                 const float* bias, const float* rscale, double* stats,
                 int M, int N, int K, int taps, int Lin, int Lout, int stride, int pad, int mode, int act,
                 hipStream_t stream);

/* C = A W^T (one tap, no bias, no activation) and, from the same epilogue, the row constants of the flash backward:
 *   delta[b][h][l] = sum_{d < 64} bf16(C[b*L + l][h*64 + d]) * O[b*L + l][h*64 + d]            (N = heads * 64, M % L == 0)
 * replaces: autograd's input-gradient of Attention.to_out (modules/unet.py:123,141) + the sum(dO * O) pass of SDPA's backward
 * (attention.py:94-99) -- i.e. osuf_gemm_nt followed by osuf_attn_delta, without re-reading dO and O. */
int osuf_gemm_nt_rowdot(int dtype, const void* A, long lda, const void* W, long ldw, void* C, long ldc, const void* O, long ldo,
                        float* delta, int M, int N, int K, int L, int heads, hipStream_t stream);

/* dW (+)= sum_m dY[m][n1] * X[rowmap(m,t)][n2].  out_layout 0: dW[t][n1][n2] with row stride ldw and tap stride tapstride;
 * out_layout 1: dense dW[n1][n2][t], i.e. torch's (Cout, Cin, k) Conv1d weight layout, so the gradient can be accumulated
 * straight into the parameter's .grad.  accumulate 1: add into dW; 0: overwrite (no zero-init needed by the caller).
 * The reduction over m is split across workgroups.  With a caller-provided fp32 `workspace` of at least
 * osuf_gemm_tn_workspace_bytes(...) bytes the partial tiles are written with plain stores and summed by a second kernel
 * (deterministic); without it (NULL / too small / shape not eligible) partial sums are added with fp32 atomics.
 * replaces: autograd's weight-gradient of every Conv1d / Linear listed above. */
int osuf_gemm_tn(int dtype, const void* dY, long ldy, const void* X, long ldx, float* dW, long ldw, long tapstride,
                 int M, int N1, int N2, int taps, int Lin, int Lout, int stride, int pad, int mode,
                 int splits, int out_layout, int accumulate, float* workspace, long workspace_bytes, hipStream_t stream);
long osuf_gemm_tn_workspace_bytes(int dtype, int M, int N1, int N2, int taps);
/* osuf_gemm_tn + the bias gradient of the same layer from the same pass over dY: dbias[n1] += sum_m dY[m][n1] (fp32, N1 entries).  The
 * bf16 256x256 and merged-taps kernels sum the dY fragments they hold anyway; every other path (fp32 modes, small shapes) runs osuf_colsum
 * on dY itself (then N1 % 8 == 0 is required).
 * replaces: autograd's weight- and bias-gradient of one Conv1d / Linear (residual.py:70,115, unet.py:118-123,149-156). */
int osuf_gemm_tn_bias(int dtype, const void* dY, long ldy, const void* X, long ldx, float* dW, long ldw, long tapstride,
                      int M, int N1, int N2, int taps, int Lin, int Lout, int stride, int pad, int mode,
                      int splits, int out_layout, int accumulate, float* workspace, long workspace_bytes, float* dbias, hipStream_t stream);

/* out[n] += sum_m Y[m][n]     replaces: autograd's bias-gradient of Conv1d / Linear. */
int osuf_colsum(int dtype, const void* Y, long ldy, int M, int N, float* out, hipStream_t stream);

/* ---- GroupNorm(1,C) + FiLM + SiLU (norm.hip)    replaces: Block.forward_body (modules/residual.py:75-84) ---- */
int osuf_gn_finalize(const double* stats, float* mean_rstd, int B, long count, hipStream_t stream);
/* The same statistics without atomics, from the stored conv output (one extra read of y): per-chunk sums in `partial`
 * (osuf_gn_stats_workspace_bytes(M, C, L) bytes), added in a fixed order -- identical inputs give identical bits.  Used by the
 * sampling loop (models/diffusion.py:59-77, inference_gradio.py:128) so that two calls of sample() return the same beatmap;
 * the training step keeps the statistics fused into the GEMM epilogue (osuf_gemm_nt `stats`, fp32/fp64 atomics). */
int osuf_gn_stats(int dtype, const void* y, long ldy, double* partial, float* mean_rstd, int M, int C, int L, hipStream_t stream);
long osuf_gn_stats_workspace_bytes(int M, int C, int L);
int osuf_gn_apply_fwd(int dtype, const void* y, long ldy, void* h, long ldh, const float* mean_rstd, const float* gamma,
                      const float* beta, const float* scale_shift, int M, int C, int L, hipStream_t stream);
/* osuf_gn_finalize + osuf_gn_apply_fwd in one launch: stats[b] = raw (sum, sum of squares) over count = L*C elements; the kernel
 * finalises them itself and also writes (mean, rstd) to mr_out[B][2] (needed again by osuf_gn_bwd). */
int osuf_gn_apply_fwd_stats(int dtype, const void* y, long ldy, void* h, long ldh, const double* stats, long count, float* mr_out,
                            const float* gamma, const float* beta, const float* ss, int M, int C, int L, hipStream_t stream);
/* The bit-reproducible statistics without their second launch: osuf_gn_stats_parts is stage 1 of osuf_gn_stats alone (per-chunk sums into
 * partial[B][osuf_gn_stats_workspace_bytes / 16][2]); osuf_gn_apply_fwd_parts adds a sample's chunks in a fixed order inside the apply kernel
 * (every wave the same order: same bits in every workgroup) and also writes (mean, rstd) to mr_out[B][2].  The sampling loop's path since round 5. */
int osuf_gn_stats_parts(int dtype, const void* y, long ldy, double* partial, int M, int C, int L, hipStream_t stream);
int osuf_gn_apply_fwd_parts(int dtype, const void* y, long ldy, void* h, long ldh, const double* partial, float* mr_out,
                            const float* gamma, const float* beta, const float* ss, int M, int C, int L, hipStream_t stream);
/* T1234 [B][4][C] fp32 zeroed scratch; S [B][2] scratch; dss [B][2C] (may be NULL); dgamma/dbeta accumulated into; dbias (may be
 * NULL): gradient of the bias of the conv that produced y (= column sums of dy, residual.py:77 `self.proj`), accumulated into;
 * dyy (may be NULL, needs dbias): column sums of dy*y -- the DoRA magnitude gradient's numerator (lora_layers.py:86-90).
 * dgamma == dbeta == NULL: the identity "norm" of Block(norm=False) (residual.py:71): the caller passes mean 0 / rstd 1 / gamma 1 /
 * beta 0 and the kernels drop every statistics term (dy = (1 + scale) * dh * silu'(u)). */
int osuf_gn_bwd(int dtype, const void* dh, long lddh, const void* y, long ldy, void* dy, long lddy, const float* mean_rstd,
                const float* gamma, const float* beta, const float* scale_shift, float* T1234, float* S, float* dss,
                float* dgamma, float* dbeta, float* dbias, float* dyy, int M, int C, int L, hipStream_t stream);

/* ---- LayerNorm    replaces: Attention.norm (modules/unet.py:117,127) ------------------------------------- */
int osuf_ln_fwd(int dtype, const void* x, long ldx, void* out, long ldo, float* mean_rstd, const float* gamma, const float* beta,
                int M, int C, hipStream_t stream);
int osuf_ln_bwd(int dtype, const void* dy, long lddy, const void* x, long ldx, void* dx, long lddx, const float* mean_rstd,
                const float* gamma, float* dgamma, float* dbeta, int M, int C, hipStream_t stream);

/* ---- GlobalContext gate    replaces: GlobalContext.forward_body + `h * se(h)` + residual add
 *      (modules/residual.py:29-32,135-137) ------------------------------------------------------------------ */
int osuf_rowdot(int dtype, const void* h, long ldh, const float* w, long w_stride, const float* bias, float* out,
                int M, int C, int L, hipStream_t stream);
/* GlobalContext pooling (residual.py:29-31) in ONE pass over h: p[B*L] = softmax_n(h . wk + bk) and pooled[B][C] = sum_n p[n] h[b,n,:] (fp32), by a
 * running softmax per workgroup + a second stage that adds the workgroups' partials in order (`part`: osuf_gca_pool_workspace_bytes bytes of
 * scratch).  Replaces osuf_rowdot + osuf_softmax_rows + osuf_wcolsum (two reads of h) on that path; no atomics: bit-reproducible. */
long osuf_gca_pool_workspace_bytes(int M, int C, int L);
int osuf_gca_pool(int dtype, const void* h, long ldh, const float* wk, const float* bk, float* part, float* p, float* pooled,
                  int M, int C, int L, hipStream_t stream);
int osuf_softmax_rows(float* p, int B, int L, hipStream_t stream);
/* osuf_wcolsum: out[b][c] (+)= sum_l w[b][l] * a[b][l][c] (* bmul[b][l][c]).  partial == NULL: row chunks meet by fp32 atomics in a
 * zero-initialised `out`; partial = B * ceil(L / 64) * C floats: chunk sums are stored and added in chunk order (`out` overwritten,
 * bit-reproducible -- the sampling loop's path). */
int osuf_wcolsum(int dtype, const void* a, long lda, const void* bmul, long ldb, const float* w, float* out,
                 int B, int C, int L, float* partial, hipStream_t stream);
int osuf_gate_residual(int dtype, const void* h, long ldh, const float* gate, const void* res, long ldr, void* out, long ldo,
                       int M, int C, int L, hipStream_t stream);
int osuf_gca_bwd_apply(int dtype, const void* dout, long lddo, const void* h, long ldh, void* dh, long lddh, const float* p,
                       const float* gate, const float* dpooled, const float* sdot, const float* wk, float* dlogit,
                       int M, int C, int L, float* dwk, float* dbk, float* workspace, long workspace_bytes, hipStream_t stream);
long osuf_gca_bwd_apply_workspace_bytes(int M, int C);
/* (dwk [C] / dbk [1], optional, accumulated into: sum_m dlogit[m] * h[m][:] and sum_m dlogit[m], the gradients of to_k's weight and
 *  bias (residual.py:20,29), from the h rows osuf_gca_bwd_apply already holds.  With a workspace of
 *  osuf_gca_bwd_apply_workspace_bytes the per-workgroup partials go through a slab and a small second kernel; without it
 *  (NULL / too small) thousands of workgroups add to the same C addresses with atomics, which costs 25-40 us per launch.) */

/* ---- attention (attn.hip) -----------------------------------------------------------------------------------
 * replaces: RotaryPositionEmbedding.forward + apply_rotary_pos_emb (modules/attention.py:52-58, utils.py:25-32) and
 *           the q/k/v -> bf16 casts of Attend.forward (attention.py:87-92) */
int osuf_rope_cast(int dtype, const void* in, long ld_in, void* out_bf16, long ld_out, const float* cos_tab, const float* sin_tab,
                   int M, int N, int n_rot_heads, int n_heads_total, int head_dim, hipStream_t stream);
/* as osuf_rope_cast (head_dim 64), and the first n_q_heads heads -- the queries -- are multiplied by q_mul before their bf16 rounding: with
 * q_mul = scale * log2(e) the softmax scale of attention.py:94-99 rides the one rounding the reference's bf16 cast (attention.py:87-92) performs
 * anyway, and osuf_mqa_fwd_qs / osuf_mqa_bwd_fused_qs take Qs K^T straight as log2-domain scores. */
int osuf_rope_cast_qs(int dtype, const void* in, long ld_in, void* out_bf16, long ld_out, const float* cos_tab, const float* sin_tab,
                      int M, int N, int n_rot_heads, int n_heads_total, int head_dim, float q_mul, int n_q_heads, hipStream_t stream);
int osuf_rope_bwd(int dtype, const float* in, long ld_in, void* out, long ld_out, const float* cos_tab, const float* sin_tab,
                  int M, int N, int n_rot_heads, int n_heads_total, int head_dim, hipStream_t stream);
/* replaces: the GQA repeat (modules/unet.py:135) + F.scaled_dot_product_attention (attention.py:94-99) and its backward.
 * q/k/v/dout are bf16; o is written bf16-rounded in o_dtype; lse2 = log2-domain logsumexp [B][H][N]. */
int osuf_mqa_fwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* o, long ldo, int o_dtype,
                 float* lse2, int B, int H, int N, int head_dim, float scale, hipStream_t stream);
/* Grouped-query attention forward in one launch: H query heads on G K/V heads (H % G == 0, r = H / G), the query heads and o laid out
 * GROUP-MAJOR.  Group g reads its queries at column g * r * head_dim of q, its K / V head at column g * head_dim of k / v, and writes o at
 * column g * r * head_dim and lse2 at [g][B][r][N]: the operands of G osuf_mqa_fwd calls with H = r, and the same bits in o and lse2.  The
 * group is a grid dimension of the same kernels (head dim 64 tuned, 16 / 32 / 128 generic); G == 1 is osuf_mqa_fwd itself.  There are no
 * pre-scaled-query, zero-fill or RoPE forms for groups.
 * replaces: the GQA repeat (modules/unet.py:135, mmdit.py:112-116) + F.scaled_dot_product_attention (attention.py:94-99), forward only. */
int osuf_gqa_fwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* o, long ldo, int o_dtype,
                 float* lse2, int B, int H, int G, int N, int head_dim, float scale, hipStream_t stream);
/* osuf_mqa_fwd for queries pre-scaled by scale * log2(e) (osuf_rope_cast_qs); same outputs, same lse2 convention; head_dim 64.
 * replaces: F.scaled_dot_product_attention at attention.py:94-99 (as osuf_mqa_fwd). */
int osuf_mqa_fwd_qs(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* o, long ldo, int o_dtype,
                    float* lse2, int B, int H, int N, int head_dim, float scale, hipStream_t stream);
/* osuf_mqa_fwd (qs = 0) / osuf_mqa_fwd_qs (qs = 1) that also zero-fills zero_dq[B*N][H*64] (fp32): the dQ accumulator at the head of the
 * workspace of this layer's osuf_mqa_bwd_fused* call, which then takes dq_mode | OSUF_DQ_PREZEROED.  The forward loop is bound by the vector
 * pipe with HBM idle, so the fill costs nothing there; in front of the backward sweep it is 66 us per N = 4096 layer.  head_dim 64 only. */
int osuf_mqa_fwd_zdq(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* o, long ldo, int o_dtype,
                     float* lse2, int B, int H, int N, int head_dim, float scale, int qs, float* zero_dq, hipStream_t stream);
/* The forward on UN-rotated queries: q_raw = the q block of the q|kv projection as the GEMM left it (bf16).  The kernel rotates each wave's
 * 32 x 64 query tile (rope_cos / rope_sin: [N][32] fp32), multiplies it by q_mul = scale * log2 e and rounds it to bf16 once -- osuf_rope_cast_qs'
 * arithmetic -- and stores it to q_out ([B*N][ldqo], may be NULL: inference) for osuf_mqa_bwd_fused_qs.  k / v: already rotated / cast
 * (osuf_rope_cast on those two head blocks alone: 128 of the (H + 2) * 64 columns).  zero_dq: as osuf_mqa_fwd_zdq, may be NULL.  head_dim 64.
 * Replaces the q part of `apply_rotary_pos_emb` + the cast in front of SDPA (attention.py:52-58,87-92) -- a full read + write of the q|kv rows. */
int osuf_mqa_fwd_rope(const void* q_raw, long ldq, const void* k, long ldk, const void* v, long ldv, void* o, long ldo, int o_dtype,
                      float* lse2, int B, int H, int N, int head_dim, float scale, const float* rope_cos, const float* rope_sin,
                      float q_mul, void* q_out, long ldqo, float* zero_dq, hipStream_t stream);
/* Attend(q, k, v, attn_mask) (attention.py:77-99): the reference casts the mask to bf16 and passes it to SDPA as an additive bias of
 * the scaled scores (so a bool mask adds 1.0 / 0.0 -- kept).  mask: bf16, element strides over (batch, head, query, key), 0 for a
 * broadcast dimension.  All head dims go through the generic kernel; its backward is osuf_mqa_bwd_masked.
 * It is osuf_xattn_fwd with Nk = N and a mask that must be there (OSUF_EINVAL for mask == NULL), so lse2 is required: the kernel
 * writes it unconditionally, and lse2 == NULL returns OSUF_EINVAL (earlier versions did not check it).
 * replaces: F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask) at attention.py:94-99. */
int osuf_mqa_fwd_masked(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* o, long ldo, int o_dtype,
                        float* lse2, const void* mask, long mask_b, long mask_h, long mask_q, long mask_k, int B, int H, int N,
                        int head_dim, float scale, hipStream_t stream);
/* The backward of osuf_mqa_fwd_masked: one K/V head, lse2 from that forward, delta from osuf_attn_delta.  dq ([B*N][lddq], head h at
 * h * head_dim), dk / dv ([B*N][lddk]) in out_dtype (OSUF_DT_F32 or OSUF_DT_BF16) are the gradients of the ROTATED q / k and of v (no RoPE
 * tables: the caller applies osuf_rope_bwd).  The bias restarts the scores exactly as in the forward.  dbias (may be NULL): dense fp32
 * [B][H][N][N], 16-byte aligned, receives dL/d(bias) = P (dP - delta) for every (query, key); it is never accumulated into.  Rows whose
 * every key is -inf are NaN in the forward and therefore in the backward.  It is osuf_xattn_bwd with Nk = N and a mask that must be there.
 * replaces: the backward of F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask) at attention.py:94-99. */
int osuf_mqa_bwd_masked(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, const void* dout, long lddo,
                        const float* lse2, const float* delta, const void* mask, long mask_b, long mask_h, long mask_q, long mask_k,
                        void* dq, long lddq, void* dk, void* dv, long lddk, int B, int H, int N, int head_dim, float scale,
                        int out_dtype, float* dbias, hipStream_t stream);
/* Cross-attention: osuf_mqa_fwd_masked with keys and values of their own length.  q / o: [B*Nq] rows, k / v: [B*Nk] rows, one K/V head,
 * lse2 [B][H][Nq].  mask (may be NULL: no bias): bf16, element strides over (batch, head, query, key) of a (B, H, Nq, Nk) bias, 0 for a
 * broadcast dimension.  Head dims 16, 32, 64 and 128 all run the generic kernels (no tuned path).
 * replaces: F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask) at attention.py:94-99 when k / v are longer or shorter than q. */
int osuf_xattn_fwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* o, long ldo, int o_dtype,
                   float* lse2, const void* mask, long mask_b, long mask_h, long mask_q, long mask_k, int B, int H, int Nq, int Nk,
                   int head_dim, float scale, hipStream_t stream);
/* The backward of osuf_xattn_fwd: lse2 from that forward, delta [B][H][Nq] from osuf_attn_delta with N = Nq.  dq: [B*Nq][lddq], head h at
 * h * head_dim; dk / dv: [B*Nk][lddk], summed over the H query heads; all in out_dtype (OSUF_DT_F32 or OSUF_DT_BF16).  dbias (may be NULL;
 * OSUF_EINVAL without a mask): dense fp32 [B][H][Nq][Nk], 16-byte aligned, never accumulated into.
 * replaces: the backward of F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask) at attention.py:94-99 (as osuf_xattn_fwd). */
int osuf_xattn_bwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, const void* dout, long lddo,
                   const float* lse2, const float* delta, const void* mask, long mask_b, long mask_h, long mask_q, long mask_k,
                   void* dq, long lddq, void* dk, void* dv, long lddk, int B, int H, int Nq, int Nk, int head_dim, float scale,
                   int out_dtype, float* dbias, hipStream_t stream);
int osuf_attn_delta(const void* dout, long lddo, const void* o, long ldo, int o_dtype, float* delta, int B, int H, int N,
                    int head_dim, hipStream_t stream);
/* dq / dk / dv are written in out_dtype (OSUF_DT_F32 or OSUF_DT_BF16).  rope_cos / rope_sin ([N][32] fp32, or both NULL): q and k
 * were rotated by apply_rotary_pos_emb (attention.py:52-58) before the attention; with the tables given, dq and dk come out as
 * gradients of the UN-rotated projections (the rotation's transpose rides the epilogue; dv is never rotated). */
int osuf_mqa_bwd_dq(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, const void* dout, long lddo,
                    const float* lse2, const float* delta, void* dq, long lddq, int B, int H, int N, int head_dim, float scale,
                    int out_dtype, const float* rope_cos, const float* rope_sin, int variant, hipStream_t stream);
int osuf_mqa_bwd_dkv(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, const void* dout, long lddo,
                     const float* lse2, const float* delta, void* dk, void* dv, long lddk, int B, int H, int N, int head_dim,
                     float scale, int out_dtype, const float* rope_cos, const float* rope_sin, float* workspace, long workspace_bytes,
                     int qsplit, int variant, hipStream_t stream);
/* Short sequences give the dK/dV kernel few 256-key workgroups (B=32, N=512: 64 on 256 CUs): with a 16-byte-aligned fp32 workspace
 * of this many bytes (0 = the shape does not need it) the query range is cut into 2 or 4 parts whose partial sums a finishing pass
 * adds in a fixed order (then scale, RoPE transpose, cast).  workspace NULL / too small: the unsplit kernel runs.
 * qsplit: 0 = the default split of the shape; 1..16 = force that many parts (the same value goes to osuf_mqa_bwd_dkv); a forced count is
 * brought down to the parts that get at least one 32-query block (N = 33 has two blocks: at most 2 parts). */
long osuf_mqa_bwd_dkv_workspace_bytes(int B, int N, int qsplit);

/* The whole attention backward in ONE key-stationary sweep (S, dP and the exponentials are computed once per (query, key) pair
 * instead of once in each of the two kernels above): dK / dV stay in registers; every 256-key workgroup leaves its partial dQ in
 * `workspace` -- dq_mode OSUF_DQ_ATOMIC: fp32 atomics into one [B*N][H*64] buffer (sum order not fixed: the last fp32 bits vary
 * between runs, as with autograd's own SDPA backward); OSUF_DQ_SLABS: one slab per key block in the output's element type, plain
 * stores, added in key-block order by the finishing pass (bit-reproducible, slower) -- and a finishing pass scales / un-rotates /
 * casts it into dq.  workspace:
 * osuf_mqa_bwd_fused_workspace_bytes(B, H, N, out_dtype, qsplit, dq_mode) bytes, 16-byte aligned.  dq / dk / dv, rope tables,
 * qsplit: as above.
 * replaces: the same call sites as osuf_mqa_bwd_dq + osuf_mqa_bwd_dkv (backward of attention.py:94-99 under unet.py:125-141). */
int osuf_mqa_bwd_fused(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, const void* dout, long lddo,
                       const float* lse2, const float* delta, void* dq, long lddq, void* dk, void* dv, long lddk, int B, int H,
                       int N, int head_dim, float scale, int out_dtype, const float* rope_cos, const float* rope_sin,
                       float* workspace, long workspace_bytes, int qsplit, int dq_mode, hipStream_t stream);
/* osuf_mqa_bwd_fused for queries pre-scaled by c = scale * log2(e) (q from osuf_rope_cast_qs, lse2 from osuf_mqa_fwd_qs): p = exp2(Qs K^T - lse2)
 * without a multiply (the generated 512-key loop drops 64 vector instructions per (head, 32-query block) pair); dq is still the gradient of the
 * UN-scaled rotated q (scale dS K), dk = (scale / c) dS^T Qs.  Same workspace, same arguments.
 * replaces: the backward of attention.py:94-99 under unet.py:125-141 (as osuf_mqa_bwd_fused). */
int osuf_mqa_bwd_fused_qs(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, const void* dout, long lddo,
                          const float* lse2, const float* delta, void* dq, long lddq, void* dk, void* dv, long lddk, int B, int H,
                          int N, int head_dim, float scale, int out_dtype, const float* rope_cos, const float* rope_sin,
                          float* workspace, long workspace_bytes, int qsplit, int dq_mode, hipStream_t stream);
long osuf_mqa_bwd_fused_workspace_bytes(int B, int H, int N, int out_dtype, int qsplit, int dq_mode);

/* ---- layout / scheduler / optimizer (elementwise.hip; the samplers' kernels: sampling.hip) -----------------------
 * replaces: the (B,C,L) <-> (B,L,C) rearranges (modules/unet.py:180,183) at the model boundary, torch.cat (unet.py:500,
 *           507,510), DDIMScheduler.add_noise / .step (models/diffusion.py:96,75; diffusers 0.29.2), the CFG combine
 *           (unet.py:465), F.mse_loss + mask (diffusion.py:101-111), get_total_norm / clip_grad_norm_ / AdamW.step
 *           (trainer.py:32-39,302-307).
 * OSUF_EINVAL, nothing launched: a size < 1; width, cols or a leading dimension that is no multiple of 8 (8-wide chunks); width <
 * C * KT or > ld; osuf_rows_to_ncl's ld < C; a NULL in / out / src / dst / a / b, pred / target / loss_sum, osuf_sqnorm's g / out,
 * osuf_clip_coef's sumsq / coef; a pointer off a 16-byte boundary where the kernel moves 16 bytes per access (osuf_ncl_to_rows' out,
 * osuf_copy2d's and osuf_add2d's operands, osuf_sqnorm's g, osuf_adamw's four buffers, osuf_cast_f32_bf16's src and dst); step < 1.
 * OSUF_EUNSUPPORTED: an unknown dtype code.  Checked case by case in tests/test_elementwise_rows_gpu.py. */
int osuf_ncl_to_rows(int dtype, const float* in, void* out, long ld, int width, int B, int C, int L, int KT, hipStream_t stream);
int osuf_rows_to_ncl(int dtype, const void* in, long ld, float* out, int B, int C, int L, hipStream_t stream);
int osuf_copy2d(int src_dtype, const void* src, long lds, int dst_dtype, void* dst, long ldd, int M, int cols, hipStream_t stream);
int osuf_add2d(int dtype, const void* a, long lda, const void* b, long ldb, void* dst, long ldd, int M, int cols, hipStream_t stream);
int osuf_axpby_rows(const float* x, const float* y, const float* ca, const float* cb, float* out, int B, long per_sample, hipStream_t stream);
int osuf_ddim_step(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, float* out,
                   int B, long per_sample, hipStream_t stream);
/* Continuous-time Gaussian diffusion (replaces: modules/scheduler.py:11-23, 83-93, 121-123 and the ancestral step a DDPM sampler
 * composes from them).  osuf_ct_schedule: t[B], t_next[B] or NULL, kind 0 = linear / 1 = cosine log-SNR, evaluated in fp32 in the
 * reference's order of operations -> out[B][3] = {log_snr, alpha, sigma} without t_next, else out[B][13] = those, {log_snr, alpha,
 * sigma} at t_next, c = -expm1(log_snr - log_snr_next), posterior_variance, posterior_log_variance, 1 / max(alpha, 1e-8),
 * alpha_next (1 - c) / alpha, alpha_next c, and the noise gain (t_next > 0 ? exp(0.5 posterior_log_variance) : 0).
 * osuf_ct_step: one pass over (B, per_sample) fp32 with coef = the 13-column rows: eps = nullp ? nullp + (cond - nullp) cond_scale
 * : cond; x0 = clamp((x - sigma eps) / max(alpha, 1e-8), -1, 1); out = alpha_next (x (1 - c) / alpha + c x0) + gain * noise
 * (noise may be NULL; a zero gain never reads into the result). */
int osuf_ct_schedule(const float* t, const float* t_next, int kind, float* out, int B, hipStream_t stream);
int osuf_ct_step(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, const float* noise,
                 float* out, int B, long per_sample, hipStream_t stream);
/* Prediction objectives and dynamic thresholding (Imagen 2.3) on the same rows.  objective = what the network predicts: with p = the
 * guided prediction (nullp ? nullp + (cond - nullp) cond_scale : cond) the unclamped start prediction x0 is (x - sigma p) / max(alpha, 1e-8)
 * for OSUF_CT_OBJ_NOISE, p for OSUF_CT_OBJ_X_START and alpha x - sigma p for OSUF_CT_OBJ_V.
 * osuf_ct_step_ex: osuf_ct_step with that x0 and an optional per-sample threshold, sample b's at s[b * s_ld] (s_ld = 3 reads column 2 of
 * osuf_ct_x0_quantile's rows in place): x0 = clamp(x0, -s, s) / s, else the static clamp to [-1, 1]; the posterior mean and the noise as
 * in osuf_ct_step, which is this call with OSUF_CT_OBJ_NOISE and s = NULL.
 * osuf_ct_x0_quantile: per sample, the order statistics of |x0| over its per_sample values at ranks k_lo and min(k_lo + 1, per_sample - 1)
 * (ascending, 0-based) and s = max(1, lo + (hi - lo) frac) -> out[B][3] = {lo, hi, s}.  The host passes k_lo = floor(q (per_sample - 1)) and
 * frac = q (per_sample - 1) - k_lo (torch.quantile's linear interpolation).  lo and hi are exact (a radix select on the bit patterns of
 * |x0|, x0 recomputed in every pass, nothing sorted or stored; -0.0 and subnormals in their order) and do not depend on scheduling: integer
 * histogram counts only.  workspace: osuf_ct_x0_quantile_workspace_bytes(B) bytes, 16-byte aligned, zeroed by the call; inputs finite;
 * per_sample <= 2^30, B <= 65535.  Three counting launches over (ceil(per_sample / 4096), B) workgroups and a B-workgroup finish.
 * osuf_ct_qsample: x_noisy = alpha x0 + sigma noise and (target may be NULL) the objective's training target = noise, x0 or
 * v = alpha noise - sigma x0, in one pass; sample b's alpha and sigma are sched[b * sched_ld + 1] and [+ 2] (osuf_ct_schedule's rows). */
#define OSUF_CT_OBJ_NOISE 0
#define OSUF_CT_OBJ_X_START 1
#define OSUF_CT_OBJ_V 2
int osuf_ct_step_ex(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, const float* noise,
                    int objective, const float* s, long s_ld, float* out, int B, long per_sample, hipStream_t stream);
int osuf_ct_x0_quantile(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, int objective,
                        long k_lo, float frac, float* out, void* workspace, int B, long per_sample, hipStream_t stream);
long osuf_ct_x0_quantile_workspace_bytes(int B);
int osuf_ct_qsample(const float* x0, const float* noise, const float* sched, int sched_ld, int objective, float* x_noisy, float* target,
                    int B, long per_sample, hipStream_t stream);
/* Solvers on the same log-SNR parameterisation (no counterpart in the reference, which samples ancestrally): DDIM(eta), eta in [0, 1]
 * interpolating to the ancestral sampler, and DPM-Solver++(2M) in data prediction.  Both are
 *   x_next = k_x x + k_0 x0 + k_p x0_prev + gain z,   x0 = osuf_ct_step_ex's clamped (or thresholded) start prediction.
 * osuf_ct_solver_schedule: log_snr[steps + 1], a rising fp32 grid (equal neighbours are not checked for: 2M divides by their distance) ->
 * every step's coefficients in one launch, one thread per step, fp32 without contraction as osuf_ct_schedule:
 *   rows[steps][B][13]: step i's osuf_ct_schedule row at (log_snr[i], log_snr[i + 1]), REPLICATED for the B samples, so that rows + i * B * 13
 *     is the coef of osuf_ct_x0_quantile, osuf_ct_step_ex and osuf_ct_solver_step as it stands.  Columns 0-5 and 9 by osuf_ct_schedule's
 *     expressions; 6-8, 10, 11 the ancestral c, posterior variance and log-variance, and mean factors of that pair; 12 the ancestral noise
 *     gain, zero on the last step (where osuf_ct_schedule has t_next = 0).
 *   fac[steps][4] = k_x, k_0, k_p, gain of `sampler`, ONE per step (the grid is the batch's).  With alpha, sigma at log_snr[i], _n at
 *     log_snr[i + 1], d = log_snr[i] - log_snr[i + 1], h = -d / 2:
 *     OSUF_CT_SAMPLER_DDIM: gain = sigma_eta = eta sqrt(sigma_n^2 (-expm1(d))), k_eps = sigma_n sqrt((1 - eta^2) + eta^2 exp(d))
 *       (= sqrt(sigma_n^2 - sigma_eta^2)), k_x = k_eps / sigma, k_0 = alpha_n - k_eps exp(log_snr[i] / 2), k_p = 0.
 *     OSUF_CT_SAMPLER_DPMPP_2M (eta is not read past its range check): k_d = -alpha_n expm1(-h), k_x = sigma_n / sigma, gain = 0; step 0:
 *       k_0 = k_d, k_p = 0; step i > 0, r = h_prev / h: k_0 = k_d (1 + 1 / (2r)), k_p = -k_d / (2r).
 *   OSUF_EINVAL: steps or B < 1, a NULL pointer, eta outside [0, 1]; OSUF_EUNSUPPORTED: another sampler code.
 * osuf_ct_solver_step: one pass over (B, per_sample) fp32: the guided prediction, x0 as in osuf_ct_step_ex (objective, s, s_ld as there),
 * then x_next and x0 are both written: x0 is the next step's x0_prev, so a 2M step is one launch.  coef = the step's B rows, fac = its four
 * factors.  x0_prev is read only when it is given and k_p != 0, noise only when it is given and gain != 0.  x_next and x0 must not overlap
 * each other or an input.  16-byte aligned buffers take the four-wide path, anything else the scalar one. */
#define OSUF_CT_SAMPLER_DDIM 0
#define OSUF_CT_SAMPLER_DPMPP_2M 1
int osuf_ct_solver_schedule(const float* log_snr, int steps, int sampler, float eta, float* rows, float* fac, int B, hipStream_t stream);
int osuf_ct_solver_step(const float* x, const float* cond, const float* nullp, float cond_scale, const float* coef, const float* fac,
                        const float* x0_prev, const float* noise, int objective, const float* s, long s_ld, float* x_next, float* x0, int B,
                        long per_sample, hipStream_t stream);
/* Masked generation by replacement conditioning (no counterpart in the reference): the known region of an iterate is overwritten by the
 * known signal noised to the iterate's own level, in one pass over (B, Dch, L) fp32 contiguous x, known, noise, out.
 *   mask: fp32 in [0, 1] (not checked), one row of L per sample, broadcast over the Dch channels; sample b's row starts at mask + b * mask_ld,
 *     mask_ld = 0 is one row shared by all samples.
 *   levels: a = coef[b * coef_ld + col_a], s = coef[b * coef_ld + col_s], so that rows of osuf_ct_schedule (alpha, sigma in columns 1, 2; the
 *     pair at t_next in 4, 5), of osuf_ct_solver_schedule (rows + i * B * 13) and the 4-column rows of osuf_ddim_step are read in place.
 *   tgt = a known + s noise in fp32 without contraction: two products and one sum, three roundings.  noise = NULL: tgt = a known, no noise
 *     is read.  coef = NULL: tgt = known bit for bit, neither coef nor noise is read.
 *   out = x where m == 0 and tgt where m == 1, both bit for bit (selects, not arithmetic: known and noise may hold anything, NaN included,
 *     where m == 0, x anything where m == 1, and -0.0 survives); otherwise out = x + m (tgt - x), three roundings, no contraction.
 * out == x (in place) is allowed, no other overlap.  One launch over (chunks of Dch * L, B) workgroups, plain vector stores, no allocation,
 * no host sync, graph-capturable.  The four-wide path is taken when L % 4 == 0 and x, known, noise (when read), mask and out are 16-byte
 * aligned (with mask_ld % 4 == 0, so that every mask row is); anything else takes the scalar path.
 * OSUF_EINVAL: a NULL x, known, mask or out; B, Dch or L < 1; mask_ld < 0; with coef given, coef_ld < 1 or a negative column. */
int osuf_inpaint_blend(const float* x, const float* known, const float* noise, const float* mask, long mask_ld, const float* coef, int coef_ld,
                       int col_a, int col_s, float* out, int B, int Dch, int L, hipStream_t stream);
/* Windowed sampling (osufusion_amd/windowed.py): a sequence of n >= window frames is cut into W = ceil((n - window) / stride) + 1 windows
 * of exactly `window` frames, 1 <= stride <= window; window j starts at s_j = min(j * stride, n - window), so only the last start is
 * clamped and the last window may overlap its predecessor by more than window - stride.
 *   osuf_window_gather: src fp32 (R, D, n) -> out fp32 (R * W, D, window), out[r * W + j, d, i] = src[r, d, s_j + i], a copy of bits.
 *   osuf_window_fuse: pred fp32 (R * W, D, window), weight fp32 (window), every weight > 0 (not checked) -> out fp32 (R, D, n), a tapered,
 *     normalised overlap-add.  For frame l let J(l) be the windows that cover it, in ascending j.  One window: out = pred[r * W + j, d, l - s_j]
 *     bit for bit (a select: -0.0 and NaN payloads survive, no multiply or divide).  More: num = sum_J w[l - s_j] pred[...] and
 *     den = sum_J w[l - s_j], both in fp32 in ascending j starting from the first term, every product rounded before its add (no
 *     contraction), out = num / den, one IEEE division.  A NaN in window j reaches exactly the frames that window covers.
 * Both are one launch over (chunks of a row, rows) workgroups; every output element is written by one lane: no atomics, deterministic,
 * no allocation, no host sync, graph-capturable.  out must not overlap the input.  The four-wide path is taken when n, window and stride
 * are multiples of 4 (then every start is) and every buffer is 16-byte aligned; anything else takes the scalar path.
 * OSUF_EINVAL, nothing launched: a NULL pointer; R, W, D, n or window < 1; stride < 1 or > window; n < window; W not the count above;
 * R * W beyond an int. */
int osuf_window_gather(const float* src, float* out, int R, int W, int D, int n, int window, int stride, hipStream_t stream);
int osuf_window_fuse(const float* pred, const float* weight, float* out, int R, int W, int D, int n, int window, int stride,
                     hipStream_t stream);
/* Classifier-free guidance rescale (Lin et al. 2024, sec. 3.4; no counterpart in the reference): the guided prediction brought back to the
 * conditional prediction's per-sample spread.  cond, nullp and out are fp32 (B, per_sample), contiguous; out may alias neither input.
 *   g = nullp + (cond - nullp) cond_scale in fp32, three roundings in that order (no contraction);
 *   f_b = phi sqrt(var_b(cond) / var_b(g)) + (1 - phi), var_b over the per_sample values of sample b (the estimator's normalisation cancels),
 *     from fp64 sums of c, c^2, g, g^2 as sum x^2 - (sum x)^2 / per_sample, evaluated in fp64 and rounded once -> factor[b];
 *   out = f_b g, one fp32 multiply per element.
 * f_b = 1 as a select where per_sample < 2 or var_b(g) <= 0 (all-equal predictions; exact zeros give exactly 0), and a rounding residue
 * below zero in var_b(cond) counts as zero.  NaN and Inf in a sample propagate into that sample's f_b and out and into no other sample.
 * Two launches on `stream` over (ceil(per_sample / 4096), min(B, 65535)) workgroups, no atomics: the first writes every 4096-element chunk's four
 * sums to ws[b][chunk][4] (fp64), the second adds a sample's chunks in index order, stores f_b (the sample's first workgroup) and writes its
 * chunk of out.  Chunks, lanes and the order of every sum depend on per_sample and on the path alone: sample b's bits do not depend on B or
 * on scheduling.  ws: osuf_cfg_rescale_workspace_bytes(B, per_sample) bytes, 8-byte aligned, written before it is read (no zeroing needed).
 * No allocation, no host sync, graph-capturable.  The four-wide path is taken when per_sample % 4 == 0 and cond, nullp and out are 16-byte
 * aligned; anything else takes the scalar path (a sample's sums may differ between the two in the last bits of fp64).
 * OSUF_EINVAL, nothing launched: a NULL pointer; B < 1; per_sample < 1; phi outside [0, 1] or not finite; ws not 8-byte aligned. */
long osuf_cfg_rescale_workspace_bytes(int B, long per_sample);
int osuf_cfg_rescale(const float* cond, const float* nullp, float cond_scale, float phi, void* ws, float* factor, float* out, int B,
                     long per_sample, hipStream_t stream);
/* Scaled error norm of an embedded Runge-Kutta step (the adaptive ODE samplers, osufusion_amd/ode.py; torchdiffeq's RMS norm per sample).
 * y0, y1: fp32 (B, per_sample), contiguous, the state before the step and the proposed state after it.  k, e and step are HOST arrays: S
 * device pointers to the fp32 (B, per_sample) stage derivatives, the S error weights b_j - b*_j, 1 <= S <= 7, and step = {dt, atol, rtol};
 * all three travel to the kernel by value.  Per element, in fp64:
 *   a = fma(e[j], (double)k[j][i], a) for j = 0 .. S-1 in that order from a = 0;  err = dt a;  tol = atol + rtol max(|y0_i|, |y1_i|);
 *   term = (err / tol)^2, every operation after the chain rounded on its own; term = 0 as a select where err == 0 (tol == 0 without an
 *   error is no NaN);  ratio[b] = sqrt(sum_i term / per_sample), fp64 (B,).
 * e[j] == 0 is a select: stage j is not read (it may be NULL or hold NaN).  A NaN or Inf in a stage that is read, and a NaN in y0 or
 * y1 (the maximum keeps a NaN of either state) at an element whose error is not 0, reach that sample's ratio and no other sample's.  What
 * the formula itself absorbs stays absorbed: an element whose error is exactly 0 contributes 0 whatever its states hold, and an infinite
 * state makes an infinite tolerance, so a finite error there contributes 0 too.  Two launches on `stream`, no atomics: the first, over (ceil(per_sample / 4096), min(B, 65535))
 * workgroups, writes every 4096-element chunk's sum to ws[b][chunk] (fp64), the second adds a sample's chunks in index order and writes
 * ratio[b].  Chunks, lanes and the order of every sum depend on per_sample and on the path alone: sample b's bits do not depend on B or on
 * scheduling.  ws: osuf_rk_error_workspace_bytes(B, per_sample) bytes, 8-byte aligned, written before it is read.  No allocation, no host
 * sync, graph-capturable.  The four-wide path is taken when per_sample % 4 == 0 and y0, y1 and every stage that is read are 16-byte aligned;
 * anything else takes the scalar path (a sample's sum may differ between the two in the last bits of fp64).
 * OSUF_EINVAL, nothing launched: a NULL y0, y1, k, e, step, ws or ratio; a NULL stage under a non-zero weight; S outside 1..7; B < 1;
 * per_sample < 1; a NaN weight; dt, atol or rtol not finite; atol < 0; rtol < 0; atol == rtol == 0; ws not 8-byte aligned. */
long osuf_rk_error_workspace_bytes(int B, long per_sample);
int osuf_rk_error(const float* y0, const float* y1, const float* const* k, const double* e, int S, const double* step, void* ws,
                  double* ratio, int B, long per_sample, hipStream_t stream);
int osuf_mse(const float* pred, const float* target, const int* orig_len, float* grad, double* loss_sum, int B, int Dch, int L,
             hipStream_t stream);
/* osuf_mse with per-sample weights w[B] (min-SNR-gamma): loss_sum += sum_b w[b] sum_{d, l < len_b} (pred - target)^2 and
 * grad = 2 w[b] mask (pred - target); the caller divides both by sum_b Dch len_b as for osuf_mse.  w of ones gives osuf_mse's bits. */
int osuf_mse_w(const float* pred, const float* target, const int* orig_len, const float* w, float* grad, double* loss_sum, int B, int Dch,
               int L, hipStream_t stream);
int osuf_sqnorm(const float* g, long n, double* out, hipStream_t stream);
int osuf_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, float wd,
               int step, const float* gscale, hipStream_t stream);
/* Exponential moving averages of the weights, kept in the optimizer pass.  ema holds `tracks` buffers (1..4): track j is ema + j * ema_ld,
 * n floats; ema_ld >= n, the rest of a row is padding and is never touched.  d_j = 1 - beta_j (d_j for j >= tracks is ignored).
 *   osuf_adamw_ema: osuf_adamw's effect on p, m, v bit for bit (the same device function), then, from the parameter value just written,
 *                   e_j <- fma(d_j, p_new - e_j, e_j) for every track: one more read and one more write per element and track.
 *   osuf_ema_update: the same track update (the same device function: the same bits) from p as it stands, no optimizer.
 * Two values of d_j are selects: d_j == 0 neither reads nor writes track j, d_j >= 1 stores p_new itself without reading the track.
 * Four-wide body, scalar tail (n % 4 elements), as osuf_adamw.  OSUF_EINVAL, nothing launched: tracks outside 1..4; ema_ld < n; a NULL
 * ema; a d_j < 0 or NaN; what osuf_adamw rejects; and, when n >= 4 (the four-wide path runs), an ema or an ema_ld that is not 16-byte
 * aligned (ema_ld % 4 != 0).
 *   osuf_swap: a <-> b, n floats each, in place.  OSUF_EINVAL: a == b or overlapping ranges, NULL, n < 1, a pointer not 16-byte aligned. */
int osuf_adamw_ema(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, float wd,
                   int step, const float* gscale, float* ema, long ema_ld, int tracks, float d0, float d1, float d2, float d3,
                   hipStream_t stream);
int osuf_ema_update(const float* p, float* ema, long ema_ld, long n, int tracks, float d0, float d1, float d2, float d3,
                    hipStream_t stream);
int osuf_swap(float* a, float* b, long n, hipStream_t stream);
/* Linear combination of K fp32 buffers of n elements in fp64 (post-hoc EMA reconstruction from snapshots).  src and w are HOST arrays of
 * K device pointers and K weights, 1 <= K <= 8; they travel to the kernel by value.  Per element a = (flags & 1) ? acc[i] : 0, then
 * a = fma(w[k], (double)src[k][i], a) for k = 0 .. K-1 in that order (one rounding per step); acc[i] = a if acc is not NULL and
 * out[i] = (float)a if out is not NULL.  The chain is sequential and fp64 is stored exactly: a source list cut into several calls (flags
 * = 1 on all but the first) gives the bits of one call.  w[k] == 0 is a select: source k is not read (it may be NULL or hold NaN) and a
 * stays as it is.  Four elements per lane when every source and out are 16-byte aligned and acc is 32-byte aligned, one per lane
 * otherwise, with the same bits.  n == 0 launches nothing.  OSUF_EINVAL, nothing launched: K outside 1..8, n < 0, a NaN weight, a NULL
 * source under a non-zero weight, acc and out both NULL, flags & 1 with a NULL acc. */
int osuf_lincomb(const float* const* src, const double* w, int K, double* acc, float* out, long n, int flags, hipStream_t stream);
int osuf_clip_coef(const double* sumsq, float max_norm, float base, float* coef, float* total_norm, hipStream_t stream);
int osuf_cast_f32_bf16(const float* src, void* dst, long n, hipStream_t stream);
/* GEMM operand layouts of one conv / linear weight, both from the fp32 master (O, I, k) in one pass -- what the reference gets
 * for free from cuDNN's filter transforms inside F.conv1d / its backward (modules/unet.py:61-101, residual.py:75-137):
 *   F[t][o][i] = w[o][i][t]                                (forward operand, [taps][N=O][K=I]; may be NULL)
 *   D[t'][i][o]: dkind 0 flipped taps (same conv), 1 Downsample dgrad (4 taps, tap 3 = reflected column), 2 Upsample dgrad
 *                (4 taps [w2, w1+w2, w0+w1, w0]); dkind 1/2 need k == 3.  (may be NULL)
 * out_dtype OSUF_DT_*; f_ld / d_ld = row strides and *_tapstride = tap strides of the destinations, in elements. */
int osuf_pack_weight(const float* w, int O, int I, int k, int out_dtype, void* F, long f_ld, long f_tapstride, void* D, long d_ld,
                     long d_tapstride, int dkind, hipStream_t stream);

/* The same pack for MANY weights in one launch (after an optimizer step every packed operand of the model is stale at once).
 * descs: DEVICE array of n descriptors, one per weight, fields as osuf_pack_weight's arguments; block0 = running sum of
 * ceil(O/32) * ceil(I/32) over the preceding descriptors (descs[0].block0 == 0), total_blocks = that sum over all n.
 * All destinations share out_dtype.  The table is only read: it can be built once and reused while the pointers stay put. */
typedef struct osuf_pack_desc {
  const float* w;
  void* F;
  void* D;
  long f_ld, f_tapstride, d_ld, d_tapstride;
  int O, I, k, dkind;
  int block0, reserved;
} osuf_pack_desc;                                   /* 80 bytes */
int osuf_pack_weight_group(const osuf_pack_desc* descs, int n, int total_blocks, int out_dtype, hipStream_t stream);

/* LoRA / DoRA adapters folded into an effective weight (reference: osu_fusion/modules/lora_layers.py:16-26 get_weight_norm,
 * :72-92 DoraConv1dLayer.forward, :284-298 get_delta_weight; peft 0.12 DoraLinearLayer for attn.to_q / attn.to_kv as wired at
 * trainer_peft.py:236-244).  W (O, IK) fp32 frozen base, A (r, IK), B (O, r), mag (O) or NULL for plain LoRA, IK = in*k:
 *   V = W + scaling * B A;   g = mag / ||V||_row  (1 without mag);   Weff = g * V.   g (O floats) may be NULL. */
int osuf_dora_effective(const float* W, const float* A, const float* B, const float* mag, int O, int IK, int r, float scaling,
                        float* Weff, float* g, hipStream_t stream);
/* The same effective weight without the full-size fp32 round trip (what the training step uses):
 *   osuf_dora_gain            g[o] = mag[o] / ||W[o] + s (BA)[o]||_2 (mag NULL: g = 1; partial = workspace of ceil(I/32)*O floats), plus
 *                             the transposed rank-r operand (s g B)^T = [r][O] in f32 (sgbt32) and bf16 (sgbt16), either may be NULL
 *   osuf_pack_weight_adapted  osuf_pack_weight of g[o] * (w + s * B A), formed tile by tile from the frozen master (g NULL: g = 1) */
int osuf_dora_gain(const float* W, const float* A, const float* B, const float* mag, int O, int I, int k, int r, float scaling,
                   float* partial, float* g, float* sgbt32, void* sgbt16, hipStream_t stream);
int osuf_pack_weight_adapted(const float* w, const float* A, const float* B, const float* g, float scaling, int r, int O, int I, int k,
                             int out_dtype, void* F, long f_ld, long f_tapstride, void* D, long d_ld, long d_tapstride, int dkind,
                             hipStream_t stream);
/* Tail of the rank-r adapter gradients in one launch: dB (+)= sg[o] * tb[o][q]; dA[q][i][t] (+)= gt[k-1-t][i][q]; and, when dm is
 * given, dm (+)= (s0 - bias * s1) / m   (tb = dy^T u, gt = x^T du per tap, s0 = sum dy*y, s1 = sum dy; bias may be NULL). */
int osuf_adapter_finish(const float* tb, const float* sg, float* dB, const float* gt, float* dA, const float* s0, const float* s1,
                        const float* bias, const float* m, float* dm, int O, int I, int k, int r, int accumulate, hipStream_t stream);

/* ---- embedding-sized linears (skinny.hip)    replaces: time_mlp / cond_mlp (modules/unet.py:356-367), the FiLM projection
 *      (residual.py:104-111,126-133) and GlobalContext's squeeze-excite MLP (residual.py:20-26,33-37) -- nn.Linear / 1x1 Conv1d on
 *      (B, features) rows.  fp32 in / out, W (N, K) fp32 master read in place; mode OSUF_DT_BF16 rounds both operands to bf16
 *      (autocast semantics), OSUF_DT_F32 is exact f32.  in_act: 0 none, 1 SiLU applied to x; out_act: 0 none, 2 sigmoid.
 *        fwd: y = out_act(in_act(x) W^T + b)
 *        bwd: dz = dy * out_act'(y); dx = (dz W) * in_act'(x) [dx may be NULL]; dW (+)= dz^T in_act(x), db += colsum(dz)
 *             [dW / db may be NULL; db needs dW]
 *      x, y, dy and dx are rows at strides of their own (ldx >= K, ldy / lddy >= N, lddx >= K; OSUF_EINVAL for lddx < K); a kernel
 *      writes the N columns of y and the K columns of dx only -- columns between the width and the stride keep what they held, also
 *      where dx is zeroed first for the atomic slices. ---- */
int osuf_skinny_fwd(int mode, const float* x, long ldx, const float* W, const float* bias, float* y, long ldy, int M, int N, int K,
                    int in_act, int out_act, hipStream_t stream);
int osuf_skinny_bwd(int mode, const float* dy, long lddy, const float* y, long ldy, const float* x, long ldx, const float* W,
                    float* dx, long lddx, float* dW, float* db, int M, int N, int K, int in_act, int out_act, int accumulate,
                    hipStream_t stream);

/* Group forms for linears that share ONE input x (M, K) -- the FiLM projections: every ResidualBlock applies
 * Sequential(SiLU, Linear(2048, 2C)) to the same embedding (residual.py:104-111, 35 of them per forward).  descs: DEVICE array.
 *   osuf_skinny_fwd_group: y_i = in_act(x) W_i^T + b_i for all i in one launch; block0 = running sum of ceil(N_i / 32).
 *   osuf_skinny_dx_group : dx = in_act'(x) * sum_i dy_i W_i (dx overwritten);      block0 = running sum of ceil(N_i / 512).
 * K and every N_i multiples of 8, rows 16-byte aligned (OSUF_EINVAL otherwise: use the per-linear entry points).  The weight
 * gradients stay per linear (osuf_skinny_bwd with dx == NULL), so each is complete as soon as its block's backward has run. */
typedef struct osuf_linear_desc {
  const float* W;          /* (N, K) fp32 master weight */
  const float* bias;       /* (N) or NULL */
  float* y;                /* forward output rows, row stride ldy */
  const float* dy;         /* backward: gradient of y, row stride lddy */
  long ldy, lddy;
  int N, block0;
} osuf_linear_desc;                                 /* 56 bytes */
int osuf_skinny_fwd_group(int mode, const float* x, long ldx, const osuf_linear_desc* descs, int n, int total_blocks, int M, int K,
                          int in_act, hipStream_t stream);
int osuf_skinny_dx_group(int mode, const osuf_linear_desc* descs, int n, int total_slices, const float* x, long ldx, float* dx, long lddx,
                         int M, int K, int in_act, hipStream_t stream);

/* ---- audio front end (audio.hip)    replaces: scripts/dataset_creator.py:36-55 load_audio's feature step,
 *      np.log(np.abs(librosa.vqt(y, sr=22050, hop_length=176, fmin=C0, n_bins=96, bins_per_octave=12)) + 1e-10)
 *      (called from trainer.py:104, trainer_peft.py:107, inference_gradio.py:56).
 *      wave_pad: zero-padded mono waveform (n_pad floats, >= (frames-1)*hop + K); bank: [2*bins][K] fp32 wavelet bank (real rows,
 *      then imaginary rows; built by osufusion_amd/audio.py); scale: [bins] = sqrt(filter length); spec_ws: frames*2*bins floats;
 *      out[k][t] = log(scale[k] * |sum_n wave_pad[t*hop + n] * (bank[k][n] + i bank[bins+k][n])| + eps), row stride ldo.
 *      hop and K multiples of 4.  osuf_vqt_logmag is the second stage alone (spec: [frames][ld >= 2*bins]). ---- */
int osuf_log_vqt(const float* wave_pad, long n_pad, const float* bank, int K, int bins, int hop, const float* scale, float eps,
                 float* spec_ws, float* out, long ldo, long frames, hipStream_t stream);
int osuf_vqt_logmag(const float* spec, long ld, float* out, long ldo, const float* scale, int bins, long frames, float eps,
                    hipStream_t stream);

/* The two helpers of librosa.vqt's octave recursion (core/constantq.py: after each octave, while the hop is even, the signal is
 * resampled by 1/2 with res_type="soxr_hq", scale=True): osuf_fir_decimate2 -- out[m] = sum_j taps[j] * in[2m + j - (ntaps-1)/2],
 * zeros outside the input, ntaps odd (the taps carry the sqrt(2)); osuf_frame_rows -- out[t][i] = in[t*hop + i] for the octaves
 * whose hop (22, 11 samples) is not a multiple of 4 and cannot be read in place by osuf_log_vqt (call it with hop = K then). */
int osuf_fir_decimate2(const float* in, long n_in, const float* taps, int ntaps, float* out, long n_out, hipStream_t stream);
int osuf_frame_rows(const float* in, long n_in, int hop, int K, float* out, long frames, hipStream_t stream);

/* Sample-rate conversion in front of the transform    replaces: librosa.load(file, sr=22050, res_type="kaiser_best")'s resampy pass
 * (scripts/dataset_creator.py:37-38).  sr_new / sr_orig = L / M in lowest terms; table: [L][T] fp32, row p = the weights of every output
 * t with t*M % L == p (both wings of resampy's windowed sinc, built by osufusion_amd/audio.py resample_plan); x_pad: the input with
 * enough zeros on both sides that no output needs an end case.
 *     y[t] = sum_j table[t*M % L][j] * x_pad[base0 + (t*M)/L + j],  t < n_out      (64-bit positions; fp32 accumulation in tap order)
 * No atomics: an output's bits do not depend on n_out or on the launch.  y may point into a larger zero-padded buffer.
 * OSUF_EINVAL: a null pointer, a non-positive size, base0 < 0 or base0 + ((n_out-1)*M)/L + T > n_pad. */
int osuf_resample(const float* x_pad, long n_pad, const float* table, int L, int M, int T, long base0, float* y, long n_out,
                  hipStream_t stream);

/* ---- .osu hit objects -> training signals (encode.hip)    replaces: the per-frame Python loops of osu_fusion/library/osu/data/hit.py
 *      (flips, extents), cursor.py (cursor_signal) and encode.py (encode_beatmap), library/augment.py's two cursor flips and the x padding
 *      of trainer.py's collate_fn.  One thread per (sample, frame), one launch per batch, no atomics, no LDS.
 *      out: fp32 contiguous (B, 6, L): HIT, SUSTAIN, SLIDER, COMBO, CURSOR_X, CURSOR_Y in [-1, 1].  Row b, frame l < len[b], is global frame
 *      g = start[b] + l of map map_idx[b], at (double)g * 176 / 22050 * 1000 ms (evaluated in that order); frames l >= len[b], and every
 *      frame of a row whose map_idx is outside [0, n_maps), hold -1.0f in all six channels.  flip (NULL: none): bit 0 changes the sign of
 *      the stored CURSOR_X, bit 1 of CURSOR_Y.  round_pos: 1 = slider positions rounded half-to-even to whole pixels as the reference does,
 *      0 = left unrounded (measurement only).  pos_px (NULL: not wanted): fp64 (B, 2, L), the cursor in osu!pixels before the division and
 *      the rounding to fp32 (0 in padding) -- what tests/test_encode_gpu.py measures the kernel's geometry with.  All selects and geometry in fp64, contraction off, one rounding to fp32 after * 2 - 1.
 *      Tables (osufusion_amd/encode.py BeatmapTable builds them; every offset is global over the N maps; none may be empty: pad with one
 *      unused entry):
 *        map_hdr int [n_maps][8]    {n_obj, obj_off, n_sus, sus_off, n_sld, sld_off, 0, 0}
 *        obj_f   double [objs][16]  {t, end_time, rounded start_x, start_y, end_x, end_y, unrounded start_x, start_y, end_x, end_y,
 *                                    slide_duration, g0 .. g4}; Line g = {ax, ay, bx, by}, Perfect g = {cx, cy, r, theta0, theta1}
 *        obj_i   int [objs][4]      {kind: 0 circle 1 spinner 2 line 3 perfect 4 bezier, new-combo objects of the map up to and including
 *                                    this one, seg_off, n_seg}; objects sorted by t within a map
 *        ivl     double [..][2]     disjoint sorted [s, e) intervals: a map's SUSTAIN list at sus_off, its SLIDER list at sld_off
 *        seg_cum double [segs]      cum_t of the segments of a Bezier slider (ascending, last 1.0); seg_i int [segs][2] {node_off, degree};
 *        nodes   double [..][2]     control points.
 *      OSUF_EINVAL: a null pointer other than flip and pos_px, n_maps, B or L <= 0, B > 65535. ---- */
int osuf_encode_signals(const int* map_hdr, int n_maps, const double* obj_f, const int* obj_i, const double* ivl, const double* seg_cum,
                        const int* seg_i, const double* nodes, const int* map_idx, const long* start, const int* len, const int* flip,
                        int round_pos, float* out, double* pos_px, int B, int L, hipStream_t stream);

/* ---- sampled signals -> hit objects (decode.hip)    replaces: the first forty lines of decode_beatmap in
 *      osu_fusion/library/osu/data/decode.py (decode_flips / decode_extents of data/hit.py, one sample at a time on the host) and the
 *      1,000 np.histogram calls of its calculate_timing_point.  Host yardstick: osufusion_amd/decode.py (object_table, np.histogram).
 * osuf_decode_objects: x fp32 contiguous (B, 6, L), rows HIT, SUSTAIN, SLIDER, COMBO, CURSOR_X, CURSOR_Y; lengths (NULL: every sample
 *      has L frames): int32 [B], only the first lengths[b] frames of sample b exist and frame lengths[b] - 1 is the end of its signal
 *      (np.gradient's one-sided end); a lengths[b] outside [2, L] gives count[b] = 0.  Outputs, all [B][cap] but count [B]: for object
 *      i < min(count[b], cap) of sample b, in ascending frame order,
 *        frame        the onset: a frame where decode_flips of the HIT row (a hit channel is +1 where x > 0, else -1: 0.0, -0.0 and
 *                     NaN give -1) has a peak, the middle of a two-frame plateau rounded down, the two end frames never;
 *        sustain_end / slider_end  the last positive frame of the SUSTAIN / SLIDER run whose last non-positive frame is the onset
 *                     (decode_extents), -1 where no run starts there or the run is still open at the end of the signal;
 *        new_combo    1 where decode_flips of the COMBO row has this frame; a combo flip at a frame that is no onset sets it on the
 *                     LAST object (the host's index -1);
 *        px, py       fp64: rint((double(x) + 1) / 2 * 512) and (... * 384), ties to even, contraction off (np.round of the host).
 *      count[b] is the true number of onsets even when it exceeds cap; no row at or past cap is written (the caller raises).  Rows
 *      from count[b] on keep what they held.  One workgroup of 1024 lanes per sample; the four sign rows as bit masks in LDS (32 KiB),
 *      the order from a popcount prefix sum.  No atomics, no allocation, no host sync, graph-capturable; the bits do not depend on
 *      the rest of the batch.
 *      OSUF_EINVAL, nothing launched: a NULL pointer other than lengths; B < 1; L < 2 or > 65536; cap < 1.
 * osuf_tempo_scan: frame / count / cap as written above (count[b] is clamped to [0, cap]; a frame outside [0, L) is skipped);
 *      frame_times fp64 [L] in ms; beat_len fp64 [B][C].  For every (b, c): the phases np.remainder(frame_times[frame], beat_len) (fmod,
 *      plus beat_len once where the remainder's sign differs) go into numpy's 100 uniform bins over [0, beat_len] -- idx = (int)(phase /
 *      beat_len * 100); 100 -> 99; one step down where phase < idx * (beat_len / 100); one step up where phase >= the next edge and
 *      idx != 99 -- and best_count[b][c] = the largest bin count, best_bin[b][c] = the index of the first bin that holds it.  One wave
 *      per candidate, integer LDS atomics only: order-independent.  No allocation, no host sync, graph-capturable.
 *      OSUF_EINVAL, nothing launched: a NULL pointer; B < 1 or > 65535; C, L or cap < 1. ---- */
int osuf_decode_objects(const float* x, const int* lengths, int B, int L, int cap, int* count, int* frame, int* sustain_end,
                        int* slider_end, int* new_combo, double* px, double* py, hipStream_t stream);
int osuf_tempo_scan(const int* frame, const int* count, int cap, const double* frame_times, int L, const double* beat_len, int B, int C,
                    int* best_count, int* best_bin, hipStream_t stream);

/* ---- DiT row kernels (dit.hip)    replaces: osu_fusion/modules/dit.py:14-15 modulate(LayerNorm(x)), 275-277 the audio statistics
 *      pooling (63-70 MultiHeadRMSNorm: osuf_joint_qknorm_fwd / _bwd below, one stream and G = H).  Rows [M][C], M = B * L, sample of row m = m / L; C % 8 == 0, C <= 2048; row strides multiples of 8
 *      elements, 16-B aligned pointers.  No atomics: every cross-row sum goes through per-workgroup partials added in a fixed order.
 * osuf_adaln_fwd: out = LN(x) * (1 + scale[b]) + shift[b] (no affine, eps given); shift / scale fp32 read at [b * ldm + c] (e.g. column
 *      blocks of the (B, 6C) modulation output, ldm = 6C); mr[2m] = mean, mr[2m+1] = rstd (fp32).
 * osuf_adaln_bwd: dx = dres + LN-backward(dy * (1 + scale[b])) (dres may be NULL); stores dshift[b][c] = sum_n dy at dmod[b * ldd + c]
 *      and dscale[b][c] = sum_n dy * xhat at dmod[b * ldd + off2 + c] (e.g. column blocks of the (B, 6C) modulation gradient, ldd = 6C);
 *      B = M / L <= 65535; workspace: osuf_adaln_bwd_workspace_bytes(M, C, L) bytes.
 * osuf_stat_pool: a fp32 (B, C, L) contiguous -> out (B, 2C) = [mean_l | unbiased std_l].
 * OSUF_EINVAL, nothing launched (as the elementwise contract above): C outside 8 .. 2048 or no multiple of 8; M, L < 1 or M % L; a row
 *      stride that is no multiple of 8 (ldm: of 4) or below C -- ldx, ldo, lddy, lddx, ldm, ldd, and ldr when dres is given; a NULL
 *      x / out / shift / scale (forward; mr may be NULL: mean and rstd are then not kept), a NULL dy / x / dx / scale / mr / dmod /
 *      workspace (backward); x, out, dy, dx, dres, shift or scale off a 16-byte boundary; B > 65535 (backward, osuf_stat_pool); a
 *      workspace smaller than osuf_adaln_bwd_workspace_bytes; osuf_stat_pool's NULL a / out or a size < 1.  OSUF_EUNSUPPORTED: an
 *      unknown dtype code.  Checked case by case, with the joint entry points below, in tests/test_dit_rows_gpu.py. ---- */
int osuf_adaln_fwd(int dtype, const void* x, long ldx, void* out, long ldo, float* mr, const float* shift, const float* scale, long ldm,
                   int M, int C, int L, float eps, hipStream_t stream);
long osuf_adaln_bwd_workspace_bytes(int M, int C, int L);
int osuf_adaln_bwd(int dtype, const void* dy, long lddy, const void* x, long ldx, const void* dres, long ldr, void* dx, long lddx,
                   const float* mr, const float* scale, long ldm, float* dmod, long ldd, long off2, float* workspace, long workspace_bytes,
                   int M, int C, int L, hipStream_t stream);
int osuf_stat_pool(const float* a, float* out, int B, int C, int L, hipStream_t stream);

/* ---- joint attention rows (dit.hip)    replaces: osu_fusion/modules/mmdit.py:99-121 (rearrange, MultiHeadRMSNorm, the GQA repeat and
 *      pack([.._a, .._x], "b h * d") of JointAttention) and 124-126 (unpack + rearrange), and autograd's transposes of them.
 *      The joint buffer holds, per sample b, Nj rows: a stream with Ns rows per sample at row offset `off` (0 <= off, off + Ns <= Nj) owns
 *      rows b * Nj + off .. + Ns - 1; M = B * Ns is the stream's row count.  Every call serves ONE stream and leaves the joint rows of
 *      the other untouched (a layer calls each entry point once per stream).  Joint columns are what osuf_mqa_* read with G K/V heads:
 *      [H q heads group-major | G k heads | G v heads], D each; natural query head j (which reads K/V head j % G, as the reference's
 *      "b h n d -> b (r h) n d" repeat has it) sits in column block (j % G) * (H / G) + j / G.  The stream side is always in natural
 *      head order.  D in {16, 32, 64, 128}, H % G == 0, (H + 2G) D <= 4096.  The DiT's fused to_qkv rows are the one-stream case
 *      Ns == Nj, off == 0, G == H: the joint rows are then the plain q|k|v rows.
 * osuf_joint_qknorm_fwd: raw q|k|v projection rows [M][(H + 2G) D] (dtype) -> bf16 joint rows; q and k heads
 *      x / max(||x||, 1e-12) * gamma[h] * sqrt(D), computed in fp32 with one bf16 rounding (gamma_q [H][D], gamma_k [G][D]),
 *      v copied; inv[m][H + G] = 1 / max(||x||, 1e-12) of the stream's q then k heads.  gamma_q == gamma_k == NULL: cast and permute
 *      only (qk_norm=False), inv unused.
 * osuf_joint_pack: a stream's rows [M][H D] (dtype, natural head order) -> its bf16 joint rows [..][H D] group-major (dO).
 * osuf_joint_unpack: the transpose: bf16 joint rows -> the stream's rows in `dtype` (the attention output).
 * osuf_joint_qknorm_bwd: fp32 dq|dk|dv joint rows -> gradient of the stream's raw projections (dtype); dgamma = [dgamma_q [H][D] |
 *      dgamma_k [G][D]] fp32 stored, summed in a fixed order; workspace: osuf_joint_qknorm_bwd_workspace_bytes(M, H, G, D) bytes.
 *      Both gammas NULL: permute and cast only (x, inv, dgamma, workspace unused). ---- */
int osuf_joint_qknorm_fwd(int dtype, const void* x, long ldx, void* y, long ldy, float* inv, const float* gamma_q, const float* gamma_k,
                          int M, int Ns, int Nj, int off, int H, int G, int D, hipStream_t stream);
int osuf_joint_pack(int dtype, const void* x, long ldx, void* joint, long ldj, int M, int Ns, int Nj, int off, int H, int G, int D,
                    hipStream_t stream);
int osuf_joint_unpack(int dtype, const void* joint, long ldj, void* out, long ldo, int M, int Ns, int Nj, int off, int H, int G, int D,
                      hipStream_t stream);
long osuf_joint_qknorm_bwd_workspace_bytes(int M, int H, int G, int D);
int osuf_joint_qknorm_bwd(int dtype, const float* g, long ldg, const void* x, long ldx, const float* inv, const float* gamma_q,
                          const float* gamma_k, void* dx, long lddx, float* dgamma, float* workspace, long workspace_bytes,
                          int M, int Ns, int Nj, int off, int H, int G, int D, hipStream_t stream);

/* Measurement aid (no reference counterpart): sustained shader clock under an MFMA (mode 1) or VALU (mode 0) load.
 * out[2*block] = shader cycles, out[2*block+1] = 100 MHz wall ticks. */
int osuf_clock_probe(int blocks, int iters, int mode, long* out, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OSUFUSION_HIP_H */
