// frames.h -- what the STFT family (stft.hip, stft_stream.hip, target.hip, stats.hip, istft.hip, istft_stream.hip) shares
// about the framed, windowed DFT: the descriptor rule, the basis formula, the inverse's formulae, the spectrum workspace and
// the transform itself.  A real DFT of every frame of a [B][L] batch is ONE fp32-MFMA GEMM,
// S[(b,t)][2f + {re,im}] = sum_k wave[b][t*hop + k] basis[k][2f + {re,im}], run through igemm::launch; it is compiled once, in
// stft.hip.
#pragma once
#include "igemm.h"

namespace frames {

// transform lengths the engine's K steps and the streaming kernel's 16-sample groups take
static inline bool ok_n_fft(int n_fft) { return n_fft >= 32 && n_fft % 32 == 0; }
static inline bool ok_desc(const avvad_stft_desc* d) {
  return d && d->B > 0 && d->L > 0 && ok_n_fft(d->n_fft) && d->hop > 0 && d->T > 0 &&
         (long)(d->T - 1) * d->hop + d->n_fft <= d->L + d->hop;   // at most the reference's one-hop end pad
}

// ---- the basis formula: periodic Hann and the exactly reduced phase, in double; a caller rounds its product once
__device__ __forceinline__ double hann(int k, int N) { return 0.5 - 0.5 * cospi(2.0 * (double)k / (double)N); }
// cos and sin of 2 pi f k / N.  An element of a basis needs one of the two, so each is evaluated where it is asked for.
struct Phase {
  double ang;   // in units of pi
  __device__ __forceinline__ double cos() const { return cospi(ang); }
  __device__ __forceinline__ double sin() const { return sinpi(ang); }
};
__device__ __forceinline__ Phase phase(int f, int k, int N) {
  const long fk = ((long)f * k) % N;                                              // exact phase reduction
  return Phase{2.0 * (double)fk / (double)N};
}

// ---- the inverse's formulae (istft.hip, istft_stream.hip)
// element (f, re | im, n) of the windowed inverse real DFT: hann[n] w_f/N cos(2 pi f n / N) | -hann[n] w_f/N sin(2 pi f n / N),
// w_f = 1 for DC and Nyquist, else 2 (irfft of a half spectrum, then the synthesis window)
__device__ __forceinline__ float idft_element(int f, bool imag, int n, int N) {
  const double win = hann(n, N);
  const double wf = (f == 0 || 2 * f == N) ? 1.0 : 2.0;
  const Phase ph = phase(f, n, N);
  return (float)(imag ? -win * (wf / (double)N) * ph.sin() : win * (wf / (double)N) * ph.cos());
}
// spectrum value v under mask value g, mode 1 .. 3: the mask itself, sigmoid(logit) or logit > 0.  SIG: mode 2, its own
// instantiation of whatever calls this, so that the exponential's registers do not weigh on the other modes.
template <bool SIG>
__device__ __forceinline__ float apply_mask(float v, float g, int mode) {
  if constexpr (SIG) return v * (1.f / (1.f + expf(-g)));
  else return v * (mode == 1 ? g : (g > 0.f ? 1.f : 0.f));
}
// the frames t0 .. t1 that cover sample sp of a stream whose last frame is `last` (none when t0 > t1)
struct Cover { long t0, t1; };
__device__ __forceinline__ Cover covering(long sp, int N, int hop, long last) {
  const long lo = sp - N + 1, hi = sp / hop;
  return Cover{lo > 0 ? (lo + hop - 1) / hop : 0, hi > last ? last : hi};
}
// librosa's normalisation of an overlap-add sum by the window sum of squares, where that exceeds float32 tiny
constexpr float F32_TINY = 1.17549435e-38f;
__device__ __forceinline__ float ola_normalise(float acc, double wss) {
  const float w = (float)wss;
  return w > F32_TINY ? acc / w : acc;
}

static inline int grid1(long n) { long b = (n + 255) / 256; return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }
// row pitch (floats) of S: the 2F interleaved (re, im) columns rounded up to a float4
static inline int spectrum_ld(int n_fft) { return (2 * (n_fft / 2 + 1) + 3) / 4 * 4; }

// The spectrum workspace [W n_fft x ld][S M x ld][engine slab], M = B*T: float offsets from the workspace's start, every
// part a multiple of 64 floats behind `base`.  A module that puts buffers of its own between S and the slab (istft.hip)
// starts them at S_end and sets `slab` to where its own carve-up has it.
struct SpecWs {
  int ld;
  size_t W, S, S_end, slab, total;
};
static inline SpecWs spec_ws(int n_fft, size_t M, size_t base = 0) {
  SpecWs w;
  w.ld = spectrum_ld(n_fft);
  w.W = base;
  w.S = w.W + align_up((size_t)n_fft * w.ld, 64);
  w.S_end = w.S + align_up(M * w.ld, 64);
  w.slab = w.S_end;
  w.total = w.slab + igemm::SLAB_FLOATS;
  return w;
}

// ws + w.S [B*T][ld] = framed, windowed DFT of wave [B][L]; w = spec_ws(n_fft, B*T, ...) within the workspace ws
int framed_dft(const float* wave, long L, int B, int T, int n_fft, int hop, float* ws, const SpecWs& w, hipStream_t s);

// ---- the second basis formula (stoi.hip): a window of W samples under an N-point transform, W <= N, some of its bins.
// The symmetric Hann of W samples without its two zero end points (numpy.hanning(W + 2)[1:-1]), in double like hann()
__device__ __forceinline__ double hann_sym(int k, int W) { return 0.5 - 0.5 * cospi(2.0 * (double)(k + 1) / (double)(W + 1)); }
// element (k, 2j | 2j + 1) of the banded basis, bin f = f0 + j: win cos(2 pi f k / N) | -win sin(2 pi f k / N) with the
// same exactly reduced phase, formed in double and rounded once
__device__ __forceinline__ float banded_element(int k, int f, bool imag, int W, int N) {
  const double win = hann_sym(k, W);
  const Phase ph = phase(f, k, N);
  return (float)(imag ? -win * ph.sin() : win * ph.cos());
}
// row pitch (floats) of the banded spectrum: 2 nf interleaved (re, im) columns rounded up to a float4
static inline int banded_ld(int nf) { return (2 * nf + 3) / 4 * 4; }
// S [R*T][ld] (ld = banded_ld(nf)): row (r, t) = the n_fft-point real DFT of frame t of rows[r] (win samples from t * hop,
// under hann_sym, zero-extended), bins f0 .. f0 + nf - 1, column 2 (f - f0) + {re, im}.  rows: R rows of pitch ld_rows floats;
// every frame lies within its row ((T - 1) hop + win <= ld_rows).  W: win x ld floats for the basis.  The same engine
// product as framed_dft, always scheduled in whole tiles: every value is one ordered fmaf chain over the win samples, so
// a row's bits depend neither on how many rows the product has nor on the CU cap.
int banded_dft(const float* rows, long ld_rows, int R, int T, int win, int n_fft, int hop, int f0, int nf, float* W, float* S,
               hipStream_t s);
// The adjoint of banded_dft's product in its frames: dframes [M][win] = dS [M][ld] . basis^T, M = R * T rows, with W the
// basis banded_dft left (the window is inside it).  One engine product over K = 2 nf (the gathers guard k < K), whole
// tiles again: every value is one ordered fmaf chain over the 2 nf columns, independent of M and of the CU cap.
int banded_dft_adjoint(const float* dS, int M, int win, int nf, const float* W, float* dframes, hipStream_t s);

}  // namespace frames
