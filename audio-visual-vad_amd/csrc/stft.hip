// stft.hip -- STFT front-end on the GPU: framing + periodic Hann + real DFT as ONE fp32-MFMA GEMM against a
// windowed cos/sin basis, then |X|^2 -> log.
//
// Replaces stft_pytorch (packages/processing/stft.py:102-151: optional one-hop zero pad at the end, Hann(n_fft),
// torch.stft(n_fft, hop, center=False)) and the callers' power / log (scripts/evaluate_audio_net.py:141-148,
// packages/data_handling.py:454-457).  A 1024-point real DFT of a frame is a [1 x 1024] x [1024 x 1026] product;
// batched over all frames of all utterances it is a GEMM with M = B*T, K = n_fft, N = 2*(n_fft/2+1) -- MFMA work
// (2.1 GFLOP per 1000 frames) instead of a butterfly network, and the framing gather (hop 256 -> every sample is
// read by 4 frames) never materialises: the A functor reads wave[b][t*hop + k] directly.
#include "frames.h"

namespace {

// A[m = (b,t)][k] = wave[b][t*hop + k]  (zero beyond the utterance: the reference's end padding)
struct FrameRows {
  static constexpr bool KCONTIG = true;
  static constexpr int VEC = 1;
  typedef igemm::NoCtx Ctx;
  const float* p;
  long L;
  int X, K, T, hop;
  __device__ __forceinline__ Ctx prep(int) const { return Ctx(); }
  __device__ __forceinline__ void load(const Ctx&, int x, int k0, int kin, float* v) const {
    const int k = k0 + kin;
    float t = 0.f;
    if (x < X && k < K) {
      const int b = x / T, fr = x - b * T;
      const long idx = (long)fr * hop + k;
      if (idx < L) t = p[(long)b * L + idx];
    }
    v[0] = t;
  }
};

// basis[k][2f] = hann[k] cos(2 pi f k / N), basis[k][2f+1] = -hann[k] sin(2 pi f k / N); columns >= 2F are zero
__global__ void dft_basis(float* __restrict__ W, int N, int F, int ld) {
  const long n = (long)N * ld;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int k = (int)(i / ld), c = (int)(i % ld);
    float v = 0.f;
    if (c < 2 * F) {
      const double win = frames::hann(k, N);
      const frames::Phase ph = frames::phase(c >> 1, k, N);
      v = (float)((c & 1) ? -win * ph.sin() : win * ph.cos());
    }
    W[i] = v;
  }
}

// out[m][f] = log(re^2 + im^2 + eps)   (or the power itself when take_log == 0)
__global__ void power_log(const float* __restrict__ S, float* __restrict__ out, long M, int F, int ld, float eps, int take_log) {
  const long n = M * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long m = i / F;
    const int f = (int)(i - m * F);
    const float2 c = *reinterpret_cast<const float2*>(S + m * ld + 2 * f);
    const float pw = c.x * c.x + c.y * c.y;
    out[i] = take_log ? logf(pw + eps) : pw;
  }
}
// the evaluate scripts' whole feature chain behind the DFT: log(re^2 + im^2 + eps) then the train-set standardisation
// (x - mean[f]) / (std[f] + eps)  (scripts/evaluate_audio_net.py:141-163) in the same pass
__global__ void power_log_standardize(const float* __restrict__ S, const float* __restrict__ mean, const float* __restrict__ stdv,
                                      float* __restrict__ out, long M, int F, int ld, float eps, float norm_eps) {
  const long n = M * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long m = i / F;
    const int f = (int)(i - m * F);
    const float2 c = *reinterpret_cast<const float2*>(S + m * ld + 2 * f);
    const float v = logf(c.x * c.x + c.y * c.y + eps);
    out[i] = (v - mean[f]) / (stdv[f] + norm_eps);
  }
}
// legacy torch.stft real view of ONE utterance: out[f][t][{re,im}]
__global__ void to_legacy_view(const float* __restrict__ S, float* __restrict__ out, int T, int F, int ld) {
  const long n = (long)T * F * 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int ri = (int)(i & 1);
    const long r = i >> 1;
    const int t = (int)(r % T), f = (int)(r / T);
    out[i] = S[(long)t * ld + 2 * f + ri];
  }
}
// out[m][f][{re,im}] = S[m][2f + {re,im}]: the workspace spectrum without its row padding
__global__ void to_complex(const float* __restrict__ S, float* __restrict__ out, long M, int F, int ld) {
  const long n = M * F * 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long m = i / (2 * F);
    out[i] = S[m * ld + (i - m * 2 * F)];
  }
}

using frames::grid1;
using frames::ok_desc;
static inline frames::SpecWs ws_of(const avvad_stft_desc* d) { return frames::spec_ws(d->n_fft, (size_t)d->B * d->T); }

}  // namespace

int frames::framed_dft(const float* wave, long L, int B, int T, int n_fft, int hop, float* ws, const SpecWs& w, hipStream_t s) {
  const int F = n_fft / 2 + 1, ld = w.ld;
  const int M = B * T;
  float* W = ws + w.W;
  hipLaunchKernelGGL(dft_basis, dim3(grid1((long)n_fft * ld)), dim3(256), 0, s, W, n_fft, F, ld);
  FrameRows a{wave, L, M, n_fft, T, hop};
  igemm::ColPlain<4> b{W, ld, ld, n_fft, 0};
  igemm::EpiStore e{ws + w.S, ld, nullptr, 0};
  return igemm::launch<128, 128>(a, b, e, M, ld, n_fft, 1, s, ws + w.slab, /*allow_bf16=*/false);
}

// ---- the banded transform (frames.h): the same product with rows of their own pitch and the second basis formula
namespace {
// A[m = (r,t)][k] = rows[r][t*hop + k]; every frame lies within its row (checked by banded_dft)
struct PitchedFrameRows {
  static constexpr bool KCONTIG = true;
  static constexpr int VEC = 1;
  typedef igemm::NoCtx Ctx;
  const float* p;
  long ld;
  int X, K, T, hop;
  __device__ __forceinline__ Ctx prep(int) const { return Ctx(); }
  __device__ __forceinline__ void load(const Ctx&, int x, int k0, int kin, float* v) const {
    const int k = k0 + kin;
    float t = 0.f;
    if (x < X && k < K) {
      const int r = x / T, fr = x - r * T;
      t = p[(long)r * ld + (long)fr * hop + k];
    }
    v[0] = t;
  }
};
// basis[k][c] = frames::banded_element(k, f0 + c / 2, c odd); columns >= 2 nf are zero
__global__ void banded_basis(float* __restrict__ W, int win, int N, int f0, int nf, int ld) {
  const long n = (long)win * ld;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int k = (int)(i / ld), c = (int)(i % ld);
    W[i] = c < 2 * nf ? frames::banded_element(k, f0 + (c >> 1), c & 1, win, N) : 0.f;
  }
}
}  // namespace

int frames::banded_dft(const float* rows, long ld_rows, int R, int T, int win, int n_fft, int hop, int f0, int nf, float* W,
                       float* S, hipStream_t s) {
  const int ld = banded_ld(nf);
  if (R <= 0 || T <= 0 || win < 32 || win % 32 || win > n_fft || hop <= 0 || f0 < 0 || nf <= 0 || f0 + nf > n_fft / 2 + 1) return AVVAD_EINVAL;
  if ((long)(T - 1) * hop + win > ld_rows || (double)R * T * ld >= 2147483648.0) return AVVAD_EINVAL;
  const int M = R * T;
  hipLaunchKernelGGL(banded_basis, dim3(grid1((long)win * ld)), dim3(256), 0, s, W, win, n_fft, f0, nf, ld);
  PitchedFrameRows a{rows, ld_rows, M, win, T, hop};
  igemm::ColPlain<4> b{W, ld, ld, win, 0};
  igemm::EpiStore e{S, ld, nullptr, 0};
  return igemm::launch<128, 128>(a, b, e, M, ld, win, 1, s, /*slab=*/nullptr, /*allow_bf16=*/false);
}

int frames::banded_dft_adjoint(const float* dS, int M, int win, int nf, const float* W, float* dframes, hipStream_t s) {
  const int ld = banded_ld(nf);
  if (M <= 0 || win < 32 || win % 32 || nf <= 0 || (double)M * ld >= 2147483648.0) return AVVAD_EINVAL;
  igemm::RowPlain a{dS, ld, M, 2 * nf, 0};
  igemm::RowPlain b{W, ld, win, 2 * nf, 0};        // element (k, n) = basis[n][k]: the basis as it is stored, read along its rows
  igemm::EpiStore e{dframes, win, nullptr, 0};
  return igemm::launch<128, 128>(a, b, e, M, win, 2 * nf, 1, s, /*slab=*/nullptr, /*allow_bf16=*/false);
}

extern "C" size_t avvad_stft_workspace(const avvad_stft_desc* d) { return ok_desc(d) ? ws_of(d).total * sizeof(float) : 0; }

static int stft_impl(const float* wave, float* out, const avvad_stft_desc* d, int mode, const float* mean, const float* stdv,
                     float norm_eps, void* wsv, size_t ws_bytes, avvad_stream_t sv);

// mode 0: out [B][T][F] = log(|X|^2 + eps);  mode 1: out [B][T][F] = |X|^2;
// mode 2 (B == 1): out [F][T][2] = legacy torch.stft real view (re, im)
extern "C" int avvad_stft(const float* wave, float* out, const avvad_stft_desc* d, int mode, void* wsv, size_t ws_bytes,
                          avvad_stream_t sv) {
  return stft_impl(wave, out, d, mode, nullptr, nullptr, 0.f, wsv, ws_bytes, sv);
}

// log-power features standardised with the train-set statistics in the DFT's epilogue pass
extern "C" int avvad_stft_features(const float* wave, const float* mean, const float* stdv, float* out,
                                   const avvad_stft_desc* d, float norm_eps, void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  if (!mean || !stdv) return AVVAD_EINVAL;
  return stft_impl(wave, out, d, 0, mean, stdv, norm_eps, wsv, ws_bytes, sv);
}

static int stft_impl(const float* wave, float* out, const avvad_stft_desc* d, int mode, const float* mean, const float* stdv,
                     float norm_eps, void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!wave || !out || !wsv || ws_misaligned(wsv) || !ok_desc(d) || mode < 0 || mode > 2 || (mode == 2 && d->B != 1)) return AVVAD_EINVAL;
  if (ws_bytes < avvad_stft_workspace(d)) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  const frames::SpecWs w = ws_of(d);
  const int F = d->n_fft / 2 + 1, ld = w.ld, M = d->B * d->T;
  float *ws = (float*)wsv, *S = ws + w.S;
  int rc = frames::framed_dft(wave, d->L, d->B, d->T, d->n_fft, d->hop, ws, w, s);
  if (rc) return rc;
  if (mode == 2) hipLaunchKernelGGL(to_legacy_view, dim3(grid1((long)d->T * F * 2)), dim3(256), 0, s, S, out, d->T, F, ld);
  else if (mean)
    hipLaunchKernelGGL(power_log_standardize, dim3(grid1((long)M * F)), dim3(256), 0, s, S, mean, stdv, out, (long)M, F, ld, d->eps,
                       norm_eps);
  else hipLaunchKernelGGL(power_log, dim3(grid1((long)M * F)), dim3(256), 0, s, S, out, (long)M, F, ld, d->eps, mode == 0);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

// out [B][T][F][2] = the complex spectrum of avvad_stft's DFT (workspace: avvad_stft_workspace)
extern "C" int avvad_stft_complex(const float* wave, float* out, const avvad_stft_desc* d, void* wsv, size_t ws_bytes,
                                  avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!wave || !out || !wsv || ws_misaligned(wsv) || !ok_desc(d)) return AVVAD_EINVAL;
  if (ws_bytes < avvad_stft_workspace(d)) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  const frames::SpecWs w = ws_of(d);
  const int F = d->n_fft / 2 + 1;
  const long M = (long)d->B * d->T;
  float *ws = (float*)wsv, *S = ws + w.S;
  const int rc = frames::framed_dft(wave, d->L, d->B, d->T, d->n_fft, d->hop, ws, w, s);
  if (rc) return rc;
  hipLaunchKernelGGL(to_complex, dim3(grid1(M * F * 2)), dim3(256), 0, s, S, out, M, F, w.ld);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
