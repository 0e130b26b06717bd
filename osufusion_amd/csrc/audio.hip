// Audio front end: log-magnitude variable-Q transform of a mono waveform, the feature the denoiser is conditioned on
// (reference: osu_fusion/scripts/dataset_creator.py:36-55 -- np.log(np.abs(librosa.vqt(...)) + 1e-10)).
//
// Direct form.  With the complex wavelet bank laid out as rows of a [2*bins][K] fp32 matrix (real parts, then imaginary
// parts, already time-reversed and centred on the host -- osufusion_amd/audio.py), frame t of the transform is
//     spec[t][j] = sum_n wave_pad[t*hop + n] * bank[j][n]
// i.e. ONE tap-GEMM whose A operand is the padded waveform read with a row stride of `hop` samples (rows overlap; nothing
// is materialised), run on the fp32 MFMA path of gemm.hip.  The kernel below then folds |.|, the per-bin sqrt(length)
// scale and the log into the (frames, 2*bins) -> (bins, frames) transpose.
#include "common.hpp"

extern "C" int osuf_gemm_nt(int dtype, const void* A, long lda, const void* W, long ldw, long tapstride,
                            void* C, long ldc, void* C2, long ldc2, const void* R, long ldr, const void* U, long ldu,
                            const float* bias, const float* rscale, double* stats,
                            int M, int N, int K, int taps, int Lin, int Lout, int stride, int pad, int mode, int act,
                            hipStream_t stream);

namespace {

constexpr int kFrames = 64;       // frames per block

// out[k][t] = log(scale[k] * |spec[t][k] + i spec[t][bins + k]| + eps)
// Reads are row-contiguous (2*bins floats per frame), writes are frame-contiguous (64 floats = 256 B per bin row);
// the transpose goes through LDS with an odd row pitch.
__global__ __launch_bounds__(256) void vqt_logmag_kernel(const float* __restrict__ spec, long ld, float* __restrict__ out,
                                                         long ldo, const float* __restrict__ scale, int bins, long frames,
                                                         float eps) {
  extern __shared__ float tile[];                          // [kFrames][2*bins + 1]
  const int cols = 2 * bins, pitch = cols + 1;
  const long t0 = (long)blockIdx.x * kFrames;
  const int nt = (int)((frames - t0) < kFrames ? (frames - t0) : kFrames);
  for (int e = threadIdx.x; e < nt * cols; e += blockDim.x) {
    const int r = e / cols, c = e - r * cols;
    tile[r * pitch + c] = spec[(t0 + r) * ld + c];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < bins * kFrames; e += blockDim.x) {
    const int k = e / kFrames, r = e - k * kFrames;
    if (r < nt) {
      const float re = tile[r * pitch + k], im = tile[r * pitch + bins + k];
      out[(long)k * ldo + t0 + r] = logf(scale[k] * sqrtf(re * re + im * im) + eps);
    }
  }
}

// Octave recursion of librosa.vqt (core/constantq.py): between octaves the signal is low-passed and decimated by 2
//   out[m] = sum_j taps[j] * in[2m + j - (ntaps-1)/2]     (zeros outside [0, n_in); taps hold the sqrt(2) of resample(scale=True))
// One output per thread, taps staged in LDS; a 4-minute song is 5.3 M samples x ~375 taps at the first stage: ~2 GFLOP, HBM-trivial.
__global__ __launch_bounds__(256) void fir_decimate2_kernel(const float* __restrict__ in, long n_in, const float* __restrict__ taps, int ntaps,
                                                            float* __restrict__ out, long n_out) {
  extern __shared__ float st[];
  for (int j = threadIdx.x; j < ntaps; j += blockDim.x) st[j] = taps[j];
  __syncthreads();
  const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_out) return;
  const long base = 2 * m - (ntaps - 1) / 2;
  float acc = 0.f;
  for (int j = 0; j < ntaps; ++j) {
    const long i = base + j;
    if (i >= 0 && i < n_in) acc = fmaf(st[j], in[i], acc);
  }
  out[m] = acc;
}

// rows[t][i] = in[t*hop + i] (0 beyond n_in): explicit framing for the low octaves, whose hops (22, 11 samples) are not 16-byte
// multiples and so cannot be read in place by the GEMM loader
__global__ __launch_bounds__(256) void frame_rows_kernel(const float* __restrict__ in, long n_in, int hop, int K, float* __restrict__ out,
                                                         long frames) {
  const long total = frames * K;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long t = e / K;
    const long i = t * hop + (e - t * K);
    out[e] = i < n_in ? in[i] : 0.f;
  }
}

// Rational-ratio resampling (resampy's windowed-sinc interpolation; reference: librosa.load(file, sr=22050, res_type="kaiser_best"),
// scripts/dataset_creator.py:37-38).  With sr_new / sr_orig = L / M in lowest terms, output t sits at input time t*M/L: its weights
// depend on t only through t*M % L, so the host tabulates one row of T weights per phase (osufusion_amd/audio.py) and
//     y[t] = sum_j table[t*M % L][j] * x_pad[base0 + (t*M)/L + j]        (positions in 64-bit integers, never t * increment)
// A workgroup takes kRun consecutive outputs, one per lane, and stages the input span they cover in LDS once (2*kRun + T floats at
// ratio 1/2); the single row of L == 1 is staged too, other rows are read through L2 (a lane's row is contiguous, 16-byte aligned).
// fp32 accumulation in tap order, plain stores, no atomics: an output's bits depend on nothing but its own taps.
constexpr int kRun = 256;
constexpr int kResampleLds = 64 * 1024;      // bytes of LDS the two staged arrays may take; a span or a row beyond it is read in place

template <bool kStage, bool kRowLds>
__global__ __launch_bounds__(kRun) void resample_kernel(const float* __restrict__ x_pad, const float* __restrict__ table, int L, int M, int T,
                                                        long base0, float* __restrict__ y, long n_out, int row_floats) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];      // [kRowLds ? T : 0] row, then [kStage ? span : 0] input
  const long t0 = (long)blockIdx.x * kRun;
  const long left = n_out - t0;
  const int nt = left < kRun ? (int)left : kRun;
  const long q0 = t0 * M / L;
  const float* __restrict__ src = x_pad + base0 + q0;
  if (kRowLds)
    for (int j = threadIdx.x; j < T; j += kRun) rs_lds[j] = table[j];
  if (kStage) {
    const int span = (int)((t0 + nt - 1) * M / L - q0) + T;
    for (int e = threadIdx.x; e < span; e += kRun) rs_lds[row_floats + e] = src[e];
  }
  if (kStage || kRowLds) __syncthreads();
  if ((int)threadIdx.x >= nt) return;
  const long tm = (t0 + threadIdx.x) * M;
  const long q = tm / L;
  const int off = (int)(q - q0);
  float acc = 0.f;
  if constexpr (kStage && kRowLds) {
    const float* xs = rs_lds + row_floats + off;
    for (int j = 0; j < T; ++j) acc = fmaf(rs_lds[j], xs[j], acc);
  } else if constexpr (kStage) {
    const float* xs = rs_lds + off;
    const float* __restrict__ w = table + (tm - q * L) * T;
    for (int j = 0; j < T; ++j) acc = fmaf(w[j], xs[j], acc);
  } else if constexpr (kRowLds) {
    const float* __restrict__ xs = src + off;
    for (int j = 0; j < T; ++j) acc = fmaf(rs_lds[j], xs[j], acc);
  } else {
    const float* __restrict__ xs = src + off;
    const float* __restrict__ w = table + (tm - q * L) * T;
    for (int j = 0; j < T; ++j) acc = fmaf(w[j], xs[j], acc);
  }
  y[t0 + threadIdx.x] = acc;
}

}  // namespace

// x_pad: the zero-padded input (n_pad floats); table: [L][T] fp32 weights, row p for the outputs with t*M % L == p;
// y[t] = sum_j table[t*M % L][j] * x_pad[base0 + (t*M)/L + j], t < n_out.  Every read index is checked here against [0, n_pad).
extern "C" int osuf_resample(const float* x_pad, long n_pad, const float* table, int L, int M, int T, long base0, float* y, long n_out,
                             hipStream_t stream) {
  if (!x_pad || !table || !y || n_pad <= 0 || n_out <= 0 || L <= 0 || M <= 0 || T <= 0 || base0 < 0) return OSUF_EINVAL;
  if (n_out > (1L << 62) / M || (n_out + kRun - 1) / kRun > 0x7fffffffL) return OSUF_EINVAL;       // t*M in 64 bits; the grid
  const long last = (n_out - 1) * M / L;
  if (base0 > n_pad - T || last > n_pad - T - base0) return OSUF_EINVAL;                            // the last output's last tap
  const long span = ((long)(kRun - 1) * M + L - 1) / L + T;                                         // floats one run can cover
  const bool row_lds = L == 1 && (long)T * 4 <= kResampleLds / 2;
  const int row_floats = row_lds ? T : 0;
  const bool stage = (span + row_floats) * 4 <= kResampleLds;
  const unsigned grid = (unsigned)((n_out + kRun - 1) / kRun);
  const size_t lds = (size_t)(row_floats + (stage ? span : 0)) * sizeof(float);
  if (stage && row_lds) resample_kernel<true, true><<<grid, kRun, lds, stream>>>(x_pad, table, L, M, T, base0, y, n_out, row_floats);
  else if (stage) resample_kernel<true, false><<<grid, kRun, lds, stream>>>(x_pad, table, L, M, T, base0, y, n_out, row_floats);
  else if (row_lds) resample_kernel<false, true><<<grid, kRun, lds, stream>>>(x_pad, table, L, M, T, base0, y, n_out, row_floats);
  else resample_kernel<false, false><<<grid, kRun, lds, stream>>>(x_pad, table, L, M, T, base0, y, n_out, row_floats);
  return osuf_launch_status();
}

extern "C" int osuf_fir_decimate2(const float* in, long n_in, const float* taps, int ntaps, float* out, long n_out, hipStream_t stream) {
  if (!in || !taps || !out || n_in <= 0 || n_out <= 0 || ntaps <= 0 || ntaps > 8192 || (ntaps & 1) == 0) return OSUF_EINVAL;
  fir_decimate2_kernel<<<(unsigned)((n_out + 255) / 256), 256, ntaps * sizeof(float), stream>>>(in, n_in, taps, ntaps, out, n_out);
  return osuf_launch_status();
}

extern "C" int osuf_frame_rows(const float* in, long n_in, int hop, int K, float* out, long frames, hipStream_t stream) {
  if (!in || !out || n_in <= 0 || hop <= 0 || K <= 0 || frames <= 0) return OSUF_EINVAL;
  long blocks = (frames * K + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  frame_rows_kernel<<<(unsigned)blocks, 256, 0, stream>>>(in, n_in, hop, K, out, frames);
  return osuf_launch_status();
}

extern "C" int osuf_vqt_logmag(const float* spec, long ld, float* out, long ldo, const float* scale, int bins, long frames,
                               float eps, hipStream_t stream) {
  if (!spec || !out || !scale || bins <= 0 || frames <= 0 || ld < 2 * bins || ldo < frames) return OSUF_EINVAL;
  const size_t lds = (size_t)kFrames * (2 * bins + 1) * sizeof(float);
  if (lds > 160 * 1024) return OSUF_EUNSUPPORTED;
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)vqt_logmag_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const unsigned grid = (unsigned)((frames + kFrames - 1) / kFrames);
  vqt_logmag_kernel<<<grid, 256, lds, stream>>>(spec, ld, out, ldo, scale, bins, frames, eps);
  return osuf_launch_status();
}

// wave_pad: the zero-padded waveform, at least (frames - 1) * hop + K floats; bank: [2*bins][K]; spec_ws: workspace of
// frames * 2*bins floats; out: [bins][ldo].  hop and K must be multiples of 4 (16-byte rows for the fp32 GEMM loader).
extern "C" int osuf_log_vqt(const float* wave_pad, long n_pad, const float* bank, int K, int bins, int hop, const float* scale,
                            float eps, float* spec_ws, float* out, long ldo, long frames, hipStream_t stream) {
  if (!wave_pad || !bank || !spec_ws || frames <= 0 || frames >= (1L << 31) || hop <= 0 || K <= 0) return OSUF_EINVAL;
  if ((frames - 1) * (long)hop + K > n_pad) return OSUF_EINVAL;       // the last frame would read past the buffer
  // what osuf_vqt_logmag would refuse is refused before the GEMM writes the workspace
  if (!out || !scale || bins <= 0 || ldo < frames) return OSUF_EINVAL;
  if ((size_t)kFrames * (2 * bins + 1) * sizeof(float) > 160 * 1024) return OSUF_EUNSUPPORTED;
  const int M = (int)frames, N = 2 * bins;
  int rc = osuf_gemm_nt(OSUF_DT_F32, wave_pad, hop, bank, K, 0, spec_ws, N, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr,
                        nullptr, M, N, K, 1, M, M, 1, 0, 0, 0, stream);
  if (rc != OSUF_OK) return rc;
  return osuf_vqt_logmag(spec_ws, N, out, ldo, scale, bins, frames, eps, stream);
}
