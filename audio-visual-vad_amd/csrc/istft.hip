// istft.hip -- masked inverse STFT on the GPU: mask x spectrum -> per-frame inverse real DFT + synthesis window as ONE
// fp32-MFMA GEMM against a windowed cos/sin basis, then a fixed-order overlap-add gather with librosa's window
// sum-of-squares normalisation.
//
// Replaces istft of packages/processing/stft.py:63-99 (librosa.core.istft: irfft of every frame, periodic Hann, overlap-add,
// division by the window sum of squares where it exceeds float32 tiny, centre trim / length fix).  The mirror of
// frames::framed_dft: Y[(b,t)][n] = sum_c A[(b,t)][c] Winv[c][n] with M = B*T, N = n_fft, K = spectrum_ld -- the same flop
// count as the forward transform.  The mask (given, sigmoid of a logit, or logit > 0) is applied while the A operand is
// loaded, so the masked spectrum never exists in memory; the spectrum is read through element strides, so the STFT's own
// workspace rows, a batched (B,T,F,2) tensor and the legacy (F,T,2) view all go in as they are.
//
// For training (avvad_istft_bwd, avvad_resynth_bwd): the adjoint with respect to the mask or its logits.  The inverse basis is
// w_f / N times the forward one, so the adjoint of the inverse GEMM is frames::framed_dft applied to the normalised cotangent
// q (overlap_add_adjoint), followed by one epilogue pass (mask_gradient); the spectrum is data and has no gradient.
#include "frames.h"
#include "reduce.h"

namespace {

// Winv[c][n]: rows 2f, 2f + 1 = frames::idft_element (f, re | im, n); rows >= 2F are zero.  win2[n] = hann[n]^2 as doubles.
__global__ void idft_basis(float* __restrict__ W, double* __restrict__ win2, int N, int F, int rows) {
  const long n_el = (long)rows * N;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_el; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i / N), n = (int)(i % N);
    const double win = frames::hann(n, N);
    W[i] = c < 2 * F ? frames::idft_element(c >> 1, c & 1, n, N) : 0.f;
    if (c == 0) win2[n] = win * win;
  }
}

// A[m = (b,t)][c] = S[b,t,c] * m(b,t,c>>1)  (zero for c >= 2F); S through element strides, (re, im) adjacent.  Offsets are
// 32-bit (the entry points check that the last element of spec and mask lies below 2^31).  SIG: frames::apply_mask's.
template <bool SIG>
struct MaskedSpec {
  static constexpr bool KCONTIG = true;
  static constexpr int VEC = 1;
  typedef igemm::NoCtx Ctx;
  const float* S;
  const float* mask;     // [B][T][F]: the mask (mode 1) or its logit (modes 2, 3)
  unsigned sb, st, sf;
  int X, T, F, mode;
  // (the row's offsets are recomputed per K tile: kept in a per-vector context they cost 16 registers of the 8-wave
  //  kernel's 128 and spilled 84 bytes per lane against 24 in this form)
  __device__ __forceinline__ Ctx prep(int) const { return Ctx(); }
  __device__ __forceinline__ void load(const Ctx&, int x, int k0, int kin, float* v) const {
    const int c = k0 + kin;
    float r = 0.f;
    if (x < X && c < 2 * F) {
      const unsigned b = (unsigned)x / (unsigned)T, t = (unsigned)x - b * (unsigned)T, f = (unsigned)c >> 1;
      r = S[b * sb + t * st + f * sf + (c & 1)];
      if (mode) r = frames::apply_mask<SIG>(r, mask[(unsigned)x * (unsigned)F + f], mode);
    }
    v[0] = r;
  }
};

// out[b][s] = scale[b] * (sum_t Y[b,t][s' - t hop]) / wss(s'),  s' = s + start, t ascending over the frames that cover s';
// no atomics: one thread gathers one sample.  Exact zeros at and beyond out_len[b] and the row's natural length.
__global__ void overlap_add(const float* __restrict__ Y, const double* __restrict__ win2, const int* __restrict__ n_frames,
                            const int* __restrict__ out_len, const float* __restrict__ scale, float* __restrict__ out, int B,
                            int T, int N, int hop, int start, int pitch) {
  const long n_el = (long)B * pitch;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_el; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / pitch), s = (int)(i % pitch);
    const int nf = row_count(n_frames, b, T);
    int len = out_len ? out_len[b] : pitch;
    len = len > pitch ? pitch : len;
    const long natural = nf > 0 ? (long)N + (long)hop * (nf - 1) - start : 0;
    float y = 0.f;
    if (s < len && s < natural) {
      const long sp = (long)s + start;
      const frames::Cover c = frames::covering(sp, N, hop, nf - 1);
      float acc = 0.f;
      double wss = 0.0;
      for (int t = (int)c.t0; t <= (int)c.t1; ++t) {
        const int n = (int)(sp - (long)t * hop);
        acc += Y[((long)b * T + t) * N + n];
        wss += win2[n];
      }
      y = frames::ola_normalise(acc, wss);
      if (scale) y *= scale[b];
    }
    out[i] = y;
  }
}

// ---- the adjoint of the masked inverse with respect to the mask (avvad_istft_bwd, avvad_resynth_bwd)
// win2[n] = hann[n]^2 as doubles, idft_basis's own values
__global__ void hann_squares(double* __restrict__ win2, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < N) {
    const double win = frames::hann(n, N);
    win2[n] = win * win;
  }
}

// The adjoint of overlap_add: q[b][s'] = scale[b] dout[b][s' - start] / w(s') where the forward wrote a sum, w the float
// overlap_add divides by (the same ascending double sum over the row's own frames); exactly 0 everywhere else, so nothing
// of dout at or behind the row's length is read.  One thread per sample of q [B][Lq], Lq = (T - 1) hop + n_fft.
__global__ void overlap_add_adjoint(const float* __restrict__ dout, const double* __restrict__ win2,
                                    const int* __restrict__ n_frames, const int* __restrict__ out_len,
                                    const float* __restrict__ scale, float* __restrict__ q, int B, int T, int N, int hop, int start,
                                    int pitch, long Lq) {
  const long n_el = (long)B * Lq;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_el; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / Lq);
    const long sp = i % Lq, s = sp - start;
    const int nf = row_count(n_frames, b, T);
    int len = out_len ? out_len[b] : pitch;
    len = len > pitch ? pitch : len;
    const long natural = nf > 0 ? (long)N + (long)hop * (nf - 1) - start : 0;
    float g = 0.f;
    if (s >= 0 && s < len && s < natural) {
      const frames::Cover c = frames::covering(sp, N, hop, nf - 1);
      double wss = 0.0;
      for (int t = (int)c.t0; t <= (int)c.t1; ++t) wss += win2[(int)(sp - (long)t * hop)];
      g = dout[(long)b * pitch + s];
      if (scale) g *= scale[b];
      g = frames::ola_normalise(g, wss);
    }
    q[i] = g;
  }
}

// dmask[b,t,f] = (w_f / N) (G_re S_re + G_im S_im), G = framed_dft(q): the adjoint of A = S g(mask) under Y = A Winv, whose
// basis is (w_f / N) times the forward transform's.  SIG (mode 2): times sigmoid'(logit).  Frames t >= n_frames[b] are
// exact zeros and neither their spectrum nor their mask is read (q is not zero under them; they may hold anything).
template <bool SIG>
__global__ void mask_gradient(const float* __restrict__ G, int ld, const float* __restrict__ S, unsigned sb, unsigned st, unsigned sf,
                              const float* __restrict__ mask, const int* __restrict__ n_frames, float* __restrict__ dmask, int B,
                              int T, int F, int N) {
  const long n_el = (long)B * T * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_el; i += (long)gridDim.x * blockDim.x) {
    const unsigned f = (unsigned)(i % F), x = (unsigned)(i / F), b = x / (unsigned)T, t = x - b * (unsigned)T;
    const int nf = row_count(n_frames, b, T);
    float r = 0.f;
    if ((int)t < nf) {
      const float2 g = *reinterpret_cast<const float2*>(G + (long)x * ld + 2 * f);
      const float* sp = S + (b * sb + t * st + f * sf);
      const float wf = (float)(((f == 0 || 2 * (int)f == N) ? 1.0 : 2.0) / (double)N);
      r = wf * (g.x * sp[0] + g.y * sp[1]);
      if constexpr (SIG) {
        const float sg = 1.f / (1.f + expf(-mask[i]));
        r *= sg * (1.f - sg);
      }
    }
    dmask[i] = r;
  }
}

using frames::grid1;

static bool ok_desc(const avvad_istft_desc* d) {
  return d && d->B > 0 && d->T > 0 && frames::ok_n_fft(d->n_fft) && d->hop > 0 && d->hop <= d->n_fft &&
         d->start >= 0 && d->start < d->n_fft && d->out_pitch > 0 && d->mask_mode >= 0 && d->mask_mode <= 3 &&
         (long)d->B * d->T * (d->n_fft / 2 + 1) < (1L << 31);       // 32-bit offsets into the mask; B T fits an int
}
// the last element the A functor reads lies below 2^31 (32-bit offsets)
static bool ok_strides(const avvad_istft_desc* d, long sb, long st, long sf) {
  if (sb < 0 || st <= 0 || sf <= 0 || sb >= (1L << 31) || st >= (1L << 31) || sf >= (1L << 31)) return false;
  const double last = (double)(d->B - 1) * sb + (double)(d->T - 1) * st + (double)(d->n_fft / 2) * sf + 1;
  return last < 2147483648.0;
}

// workspace of the inverse: [Winv ld x n_fft][Y B*T x n_fft][win2 n_fft doubles][slab]
struct Carve {
  size_t winv, y, win2, slab, total;   // float offsets; total in floats
};
static Carve carve(const avvad_istft_desc* d, size_t base) {
  const size_t ld = frames::spectrum_ld(d->n_fft);
  Carve c;
  c.winv = base;
  c.y = c.winv + align_up(ld * d->n_fft, 64);
  c.win2 = c.y + align_up((size_t)d->B * d->T * d->n_fft, 64);
  c.slab = c.win2 + align_up((size_t)2 * d->n_fft, 64);
  c.total = c.slab + igemm::SLAB_FLOATS;
  return c;
}
static int inverse(const float* spec, long sb, long st, long sf, const float* mask, const int* n_frames, const int* out_len,
                   const float* scale, float* out, const avvad_istft_desc* d, float* ws, const Carve& c, hipStream_t s) {
  const int N = d->n_fft, F = N / 2 + 1, ld = frames::spectrum_ld(N), M = d->B * d->T;
  float* Winv = ws + c.winv;
  float* Y = ws + c.y;
  double* win2 = reinterpret_cast<double*>(ws + c.win2);
  hipLaunchKernelGGL(idft_basis, dim3(grid1((long)ld * N)), dim3(256), 0, s, Winv, win2, N, F, ld);
  igemm::ColPlain<4> b{Winv, N, N, ld, 0};
  igemm::EpiStore e{Y, N, nullptr, 0};
  int rc;
  if (d->mask_mode == 2) {
    MaskedSpec<true> a{spec, mask, (unsigned)sb, (unsigned)st, (unsigned)sf, M, d->T, F, d->mask_mode};
    rc = igemm::launch<128, 128>(a, b, e, M, N, ld, 1, s, ws + c.slab, /*allow_bf16=*/false);
  } else {
    MaskedSpec<false> a{spec, mask, (unsigned)sb, (unsigned)st, (unsigned)sf, M, d->T, F, d->mask_mode};
    rc = igemm::launch<128, 128>(a, b, e, M, N, ld, 1, s, ws + c.slab, /*allow_bf16=*/false);
  }
  if (rc) return rc;
  hipLaunchKernelGGL(overlap_add, dim3(grid1((long)d->B * d->out_pitch)), dim3(256), 0, s, Y, win2, n_frames, out_len, scale, out,
                     d->B, d->T, N, d->hop, d->start, d->out_pitch);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

// workspace of the adjoint: [W n_fft x ld][G B*T x ld][q B x Lq][win2 n_fft doubles][slab]; `W`: a forward basis the
// caller's own carve-up already holds (avvad_resynth_bwd), else it comes first
struct BwdCarve {
  frames::SpecWs g;
  size_t q, win2, total;
  long Lq;
};
static BwdCarve bwd_carve(const avvad_istft_desc* d, size_t base, const frames::SpecWs* fwd) {
  BwdCarve c;
  c.Lq = (long)(d->T - 1) * d->hop + d->n_fft;
  c.g = frames::spec_ws(d->n_fft, (size_t)d->B * d->T, base);
  if (fwd) {
    c.g.W = fwd->W;
    c.g.S_end -= c.g.S - base;
    c.g.S = base;
  }
  c.q = c.g.S_end;
  c.win2 = c.q + align_up((size_t)d->B * c.Lq, 64);
  c.g.slab = c.win2 + align_up((size_t)2 * d->n_fft, 64);
  c.total = c.g.total = c.g.slab + igemm::SLAB_FLOATS;
  return c;
}
static bool ok_bwd(const avvad_istft_desc* d) {
  return ok_desc(d) && (d->mask_mode == 1 || d->mask_mode == 2) &&
         (long)d->B * ((long)(d->T - 1) * d->hop + d->n_fft) < (1L << 31);
}
static int adjoint(const float* spec, long sb, long st, long sf, const float* mask, const int* n_frames, const int* out_len,
                   const float* scale, const float* dout, float* dmask, const avvad_istft_desc* d, float* ws, const BwdCarve& c,
                   hipStream_t s) {
  const int N = d->n_fft, F = N / 2 + 1;
  float* q = ws + c.q;
  double* win2 = reinterpret_cast<double*>(ws + c.win2);
  hipLaunchKernelGGL(hann_squares, dim3((N + 255) / 256), dim3(256), 0, s, win2, N);
  hipLaunchKernelGGL(overlap_add_adjoint, dim3(grid1((long)d->B * c.Lq)), dim3(256), 0, s, dout, win2, n_frames, out_len, scale, q,
                     d->B, d->T, N, d->hop, d->start, d->out_pitch, c.Lq);
  const int rc = frames::framed_dft(q, c.Lq, d->B, d->T, N, d->hop, ws, c.g, s);
  if (rc) return rc;
  const dim3 grid(grid1((long)d->B * d->T * F));
  if (d->mask_mode == 2)
    hipLaunchKernelGGL(mask_gradient<true>, grid, dim3(256), 0, s, ws + c.g.S, c.g.ld, spec, (unsigned)sb, (unsigned)st, (unsigned)sf,
                       mask, n_frames, dmask, d->B, d->T, F, N);
  else
    hipLaunchKernelGGL(mask_gradient<false>, grid, dim3(256), 0, s, ws + c.g.S, c.g.ld, spec, (unsigned)sb, (unsigned)st, (unsigned)sf,
                       mask, n_frames, dmask, d->B, d->T, F, N);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

}  // namespace

extern "C" size_t avvad_istft_workspace(const avvad_istft_desc* d) {
  if (!ok_desc(d)) return 0;
  return carve(d, 0).total * sizeof(float);
}

extern "C" int avvad_istft(const float* spec, long stride_b, long stride_t, long stride_f, const float* mask, const int* n_frames,
                           const int* out_len, const float* scale, float* out, const avvad_istft_desc* d, void* wsv,
                           size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!spec || !out || !wsv || !ok_desc(d) || !ok_strides(d, stride_b, stride_t, stride_f) || (d->mask_mode != 0 && !mask) ||
      ((uintptr_t)wsv & 15))
    return AVVAD_EINVAL;
  if (ws_bytes < avvad_istft_workspace(d)) return AVVAD_EWORKSPACE;
  return inverse(spec, stride_b, stride_t, stride_f, mask, n_frames, out_len, scale, out, d, (float*)wsv, carve(d, 0),
                 (hipStream_t)sv);
}

static bool ok_pair(const avvad_stft_desc* sd, const avvad_istft_desc* d) {
  return frames::ok_desc(sd) && ok_desc(d) && sd->B == d->B && sd->T == d->T && sd->n_fft == d->n_fft && sd->hop == d->hop &&
         ok_strides(d, (long)d->T * frames::spectrum_ld(d->n_fft), frames::spectrum_ld(d->n_fft), 2);
}
// the fused workspace: the forward transform's [W][S], then the inverse's carve-up, whose slab both transforms use
static Carve fused(const avvad_istft_desc* d, frames::SpecWs* f) {
  *f = frames::spec_ws(d->n_fft, (size_t)d->B * d->T);
  const Carve c = carve(d, f->S_end);
  f->slab = c.slab;
  return c;
}

extern "C" size_t avvad_resynth_workspace(const avvad_stft_desc* sd, const avvad_istft_desc* d) {
  if (!ok_pair(sd, d)) return 0;
  frames::SpecWs f;
  return fused(d, &f).total * sizeof(float);
}

// framed_dft -> masked inverse -> overlap-add; the spectrum stays in the workspace
extern "C" int avvad_resynth(const float* wave, const float* mask, const int* n_frames, const int* out_len, const float* scale,
                             float* out, const avvad_stft_desc* sd, const avvad_istft_desc* d, void* wsv, size_t ws_bytes,
                             avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!wave || !out || !wsv || !ok_pair(sd, d) || (d->mask_mode != 0 && !mask) || ((uintptr_t)wsv & 15)) return AVVAD_EINVAL;
  if (ws_bytes < avvad_resynth_workspace(sd, d)) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  float* ws = (float*)wsv;
  frames::SpecWs f;
  const Carve c = fused(d, &f);
  const int rc = frames::framed_dft(wave, sd->L, sd->B, sd->T, sd->n_fft, sd->hop, ws, f, s);
  if (rc) return rc;
  return inverse(ws + f.S, (long)sd->T * f.ld, f.ld, 2, mask, n_frames, out_len, scale, out, d, ws, c, s);
}

extern "C" size_t avvad_istft_bwd_workspace(const avvad_istft_desc* d) {
  if (!ok_bwd(d)) return 0;
  return bwd_carve(d, 0, nullptr).total * sizeof(float);
}

extern "C" int avvad_istft_bwd(const float* spec, long stride_b, long stride_t, long stride_f, const float* mask,
                               const int* n_frames, const int* out_len, const float* scale, const float* dout, float* dmask,
                               const avvad_istft_desc* d, void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!spec || !mask || !dout || !dmask || !wsv || !ok_bwd(d) || !ok_strides(d, stride_b, stride_t, stride_f) ||
      ws_misaligned(wsv))
    return AVVAD_EINVAL;
  if (ws_bytes < avvad_istft_bwd_workspace(d)) return AVVAD_EWORKSPACE;
  return adjoint(spec, stride_b, stride_t, stride_f, mask, n_frames, out_len, scale, dout, dmask, d, (float*)wsv,
                 bwd_carve(d, 0, nullptr), (hipStream_t)sv);
}

// the fused adjoint's workspace: the forward transform's [W][S] of the wave, then the adjoint's carve-up, which shares W
static BwdCarve fused_bwd(const avvad_istft_desc* d, frames::SpecWs* f) {
  *f = frames::spec_ws(d->n_fft, (size_t)d->B * d->T);
  const BwdCarve c = bwd_carve(d, f->S_end, f);
  f->slab = c.g.slab;
  return c;
}

extern "C" size_t avvad_resynth_bwd_workspace(const avvad_stft_desc* sd, const avvad_istft_desc* d) {
  if (!ok_pair(sd, d) || !ok_bwd(d)) return 0;
  frames::SpecWs f;
  return fused_bwd(d, &f).total * sizeof(float);
}

// framed_dft(wave) again (the forward kept no spectrum), then the adjoint: two forward-size GEMMs
extern "C" int avvad_resynth_bwd(const float* wave, const float* mask, const int* n_frames, const int* out_len,
                                 const float* scale, const float* dout, float* dmask, const avvad_stft_desc* sd,
                                 const avvad_istft_desc* d, void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!wave || !mask || !dout || !dmask || !wsv || !ok_pair(sd, d) || !ok_bwd(d) || ws_misaligned(wsv)) return AVVAD_EINVAL;
  if (ws_bytes < avvad_resynth_bwd_workspace(sd, d)) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  float* ws = (float*)wsv;
  frames::SpecWs f;
  const BwdCarve c = fused_bwd(d, &f);
  const int rc = frames::framed_dft(wave, sd->L, sd->B, sd->T, sd->n_fft, sd->hop, ws, f, s);
  if (rc) return rc;
  return adjoint(ws + f.S, (long)sd->T * f.ld, f.ld, 2, mask, n_frames, out_len, scale, dout, dmask, d, ws, c, s);
}
