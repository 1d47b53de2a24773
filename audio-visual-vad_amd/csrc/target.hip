// target.hip -- training labels from clean speech on the GPU: the framed-energy VAD and the ideal binary mask (IBM).
//
// Replaces packages/processing/target.py of the reference:
//   clean_speech_VAD (:5-56)               E_t = sum_k y[t*hop + k]^2 over the (end-padded, optionally centred) frames,
//                                          vad_t = E_t > 10**vad_threshold * min_t E_t           (per utterance)
//   clean_speech_IBM (:58-70)              20 log10(|S| + eps) > max(20 log10(|S| + eps)) - ibm_threshold
//                                          <=>  |S| > (max|S| + eps) * 10**(-ibm_threshold/20) - eps (per utterance)
//   noise_robust_clean_speech_IBM (:72-107)  IBM * VAD, broadcast over frequency
//   noise_aware_IBM (:151-202), threshold_IBM (:205-251)   speech and noise masks from a speech and a noise spectrum (or a
//                                          constant noise power), and the ideal ratio mask of the same pair
// The reference computes them offline, one utterance at a time, into HDF5 files (scripts/create_audio_train_files.py);
// here a ragged batch wave [B][L] (zero-padded rows, per-utterance sample and frame counts in device arrays) gets its
// labels in the training step.  Every reduction stays inside one utterance and frames t >= T_b are written as zeros.
//
// Kernel forms (all memory-bound):
//   VAD: segment_energy sums squares in fp64 (a float32 square is exact in double) over hop-sized blocks when
//        n_fft % hop == 0 -- each sample is read once -- or over whole frames otherwise, one wave per segment with
//        float4 loads on the interior of the signal and the framing functor (centre offset, reflect / zero padding,
//        zero past the utterance) at its edges; vad_decide (one workgroup per utterance) adds R = n_fft/hop blocks per
//        frame in a fixed order, takes the minimum through cross-lane + LDS reductions (reduce.h) and thresholds in
//        double.
//   IBM: the DFT is the STFT front-end's GEMM (frames.h); spectrum_max takes the per-utterance maximum of |X|^2 in one
//        pass over S (float4 loads, block reduction, one integer atomicMax per workgroup on the bit pattern of a
//        non-negative double: order-independent, so bit-reproducible); ibm_mask thresholds every bin in a second pass
//        (float4 stores), times the utterance's VAD when `robust`.
//   Noise-aware masks: one DFT GEMM per wave with the batch's own (B, T) (the bits of avvad_stft_complex), then
//        noise_aware_mask, one pass over the two spectra in ibm_mask's form: every step in double, per-bin thresholds from
//        two host tables, up to three outputs; a pure function of its inputs.
#include <math.h>

#include "frames.h"
#include "reduce.h"

namespace {

constexpr int SEGS_PER_WAVE = 8;   // energy segments one wave sums in a row
constexpr int MAX_ROWS = 8;        // spectrum rows per workgroup of the maximum pass

// padded index j of one utterance -> sample: centre offset `off`, reflect (mode 1) or zero padding, zero past the
// utterance.  n = samples after the reference's one-hop end pad (the reflection point), nread = what the row holds.
__device__ __forceinline__ float sample_at(const float* row, long j, long off, long n, long nread, int mode) {
  long s = j - off;
  if (mode == 1) {
    if (s < 0) s = -s;
    if (s >= n) s = 2 * (n - 1) - s;
  }
  return (s >= 0 && s < nread) ? row[s] : 0.f;
}

// E[b][j] = sum_{k < seg} y_b[j*stride + k]^2 (fp64) for the T_b + R - 1 segments of utterance b
__global__ void __launch_bounds__(256)
    segment_energy(const float* __restrict__ wave, long pitch, const int* __restrict__ n_samples, const int* __restrict__ n_frames,
                   int Tp, int off, int mode, int seg, int stride, int R, int nseg_pitch, int vec, double* __restrict__ E) {
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int T = row_count(n_frames, b, Tp);
  const int nseg = T > 0 ? T + R - 1 : 0;
  const long n = n_samples[b], nread = min(n, pitch);
  const float* row = wave + (long)b * pitch;
  const int j0 = blockIdx.x * (4 * SEGS_PER_WAVE), j1 = min(nseg, j0 + 4 * SEGS_PER_WAVE);
  for (int j = j0 + wv; j < j1; j += 4) {
    const long p0 = (long)j * stride;
    double acc = 0.0;
    for (int k = lane * 4; k < seg; k += 256) {
      const long s0 = p0 + k - off;
      float v0, v1, v2, v3;
      if (vec && k + 3 < seg && s0 >= 0 && s0 + 3 < nread && (s0 & 3) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(row + s0);
        v0 = q.x, v1 = q.y, v2 = q.z, v3 = q.w;
      } else {
        v0 = sample_at(row, p0 + k, off, n, nread, mode);
        v1 = k + 1 < seg ? sample_at(row, p0 + k + 1, off, n, nread, mode) : 0.f;
        v2 = k + 2 < seg ? sample_at(row, p0 + k + 2, off, n, nread, mode) : 0.f;
        v3 = k + 3 < seg ? sample_at(row, p0 + k + 3, off, n, nread, mode) : 0.f;
      }
      acc += (double)v0 * v0;
      acc += (double)v1 * v1;
      acc += (double)v2 * v2;
      acc += (double)v3 * v3;
    }
    acc = wave_sum(acc);
    if (lane == 0) E[(long)b * nseg_pitch + j] = acc;
  }
}

__device__ __forceinline__ double frame_energy(const double* e, int t, int R) {
  double s = 0.0;
  for (int r = 0; r < R; ++r) s += e[t + r];
  return s;
}

// vad[b][t] = E_t > coef * min_t E_t  for t < T_b, 0 for T_b <= t < Tp.  One workgroup per utterance.
__global__ void __launch_bounds__(256)
    vad_decide(const double* __restrict__ E, int nseg_pitch, const int* __restrict__ n_frames, int R, double coef, int Tp, int vec,
               float* __restrict__ vad) {
  __shared__ double red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = row_count(n_frames, b, Tp);
  const double* e = E + (long)b * nseg_pitch;
  double mn = __builtin_huge_val();
  for (int t = tid; t < T; t += 256) mn = fmin(mn, frame_energy(e, t, R));
  const auto least = [](double a, double b) { return fmin(a, b); };
  fold4_put(red, mn, least);
  __syncthreads();
  const double thr = coef * fold4_get(red, least);
  float* out = vad + (long)b * Tp;
  if (vec) {                                               // Tp % 4 == 0 and a 16-byte aligned output
    for (int t4 = tid * 4; t4 < Tp; t4 += 1024) {
      float v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = (t4 + q < T && frame_energy(e, t4 + q, R) > thr) ? 1.f : 0.f;
      *reinterpret_cast<float4*>(out + t4) = make_float4(v[0], v[1], v[2], v[3]);
    }
  } else {
    for (int t = tid; t < Tp; t += 256) out[t] = (t < T && frame_energy(e, t, R) > thr) ? 1.f : 0.f;
  }
}

__device__ __forceinline__ double block_max_256(double mx) {
  __shared__ double red[4];
  const auto most = [](double a, double b) { return fmax(a, b); };
  fold4_put(red, mx, most);
  __syncthreads();
  return fold4_get(red, most);
}

// maxbits[b] = max over the rows t < T_b of S [B*Tp][ld] of re^2 + im^2 (the zero pad columns add nothing)
__global__ void __launch_bounds__(256)
    spectrum_max(const float* __restrict__ S, int ld, int Tp, const int* __restrict__ n_frames, unsigned long long* __restrict__ maxbits) {
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * MAX_ROWS;
  const int nr = min(row_count(n_frames, b, Tp) - t0, MAX_ROWS);
  if (nr <= 0) return;                                     // uniform across the workgroup
  const int n4 = ld >> 2;
  const float4* p = reinterpret_cast<const float4*>(S + ((long)b * Tp + t0) * ld);   // nr contiguous rows
  double mx = 0.0;
  for (int i = threadIdx.x; i < nr * n4; i += 256) {
    const float4 q = p[i];
    mx = fmax(mx, fmax((double)q.x * q.x + (double)q.y * q.y, (double)q.z * q.z + (double)q.w * q.w));
  }
  mx = block_max_256(mx);
  if (threadIdx.x == 0) atomicMax(maxbits + b, (unsigned long long)__double_as_longlong(mx));
}

// |S| > tau  <=>  |S|^2 > tau^2 with tau = (max|S| + eps) * coef - eps; tau < 0 (e.g. an all-zero spectrum) passes every bin
__device__ __forceinline__ double mask_tau(const unsigned long long* maxbits, int b, double coef, double eps) {
  return (sqrt(__longlong_as_double((long long)maxbits[b])) + eps) * coef - eps;
}
__device__ __forceinline__ float mask_bit(float re, float im, double tau) {
  return (tau < 0.0 || (double)re * re + (double)im * im > tau * tau) ? 1.f : 0.f;
}

// out [B][Tp][F] (batch-first labels): four consecutive outputs per thread, one float4 store
__global__ void __launch_bounds__(256)
    ibm_mask(const float* __restrict__ S, int ld, int F, int Tp, int B, const int* __restrict__ n_frames,
             const unsigned long long* __restrict__ maxbits, double coef, double eps, const float* __restrict__ vad, int vec,
             float* __restrict__ out) {
  const long n = (long)B * Tp * F, n4 = (n + 3) >> 2;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < n4; g += (long)gridDim.x * 256) {
    const long i = g * 4;
    long m = i / F;
    int f = (int)(i - m * F);
    int b = (int)(m / Tp), t = (int)(m - (long)b * Tp);
    int Tb = row_count(n_frames, b, Tp);
    double tau = mask_tau(maxbits, b, coef, eps);
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float r = 0.f;
      if (i + q < n && t < Tb) {
        const float2 c = *reinterpret_cast<const float2*>(S + m * ld + 2 * f);
        r = mask_bit(c.x, c.y, tau);
        if (vad) r *= vad[(long)b * Tp + t];
      }
      v[q] = r;
      if (++f == F) {                                      // next spectrum row (and maybe the next utterance)
        f = 0, ++m;
        if (++t == Tp && i + q + 1 < n) t = 0, ++b, Tb = row_count(n_frames, b, Tp), tau = mask_tau(maxbits, b, coef, eps);
      }
    }
    if (vec && i + 3 < n) *reinterpret_cast<float4*>(out + i) = make_float4(v[0], v[1], v[2], v[3]);
    else
      for (int q = 0; q < 4 && i + q < n; ++q) out[i + q] = v[q];
  }
}

// one utterance's spectrum given as interleaved (re, im) pairs at spec[t*st + f*sf]: its maximum of re^2 + im^2
__global__ void __launch_bounds__(256)
    spectrum_max_strided(const float* __restrict__ spec, long st, long sf, int T, int F, unsigned long long* __restrict__ maxbits) {
  const long n = (long)T * F;
  double mx = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long f = i / T, t = i - f * T;
    const float2 c = *reinterpret_cast<const float2*>(spec + t * st + f * sf);
    mx = fmax(mx, (double)c.x * c.x + (double)c.y * c.y);
  }
  mx = block_max_256(mx);
  if (threadIdx.x == 0) atomicMax(maxbits, (unsigned long long)__double_as_longlong(mx));
}

// out [F][T] in the caller's orientation, times vad[t] when given
__global__ void __launch_bounds__(256)
    ibm_mask_strided(const float* __restrict__ spec, long st, long sf, int T, int F, const unsigned long long* __restrict__ maxbits,
                     double coef, double eps, const float* __restrict__ vad, int vec, float* __restrict__ out) {
  const long n = (long)T * F, n4 = (n + 3) >> 2;
  const double tau = mask_tau(maxbits, 0, coef, eps);
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < n4; g += (long)gridDim.x * 256) {
    const long i = g * 4;
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float r = 0.f;
      if (i + q < n) {
        const long f = (i + q) / T, t = (i + q) - f * T;
        const float2 c = *reinterpret_cast<const float2*>(spec + t * st + f * sf);
        r = mask_bit(c.x, c.y, tau);
        if (vad) r *= vad[t];
      }
      v[q] = r;
    }
    if (vec && i + 3 < n) *reinterpret_cast<float4*>(out + i) = make_float4(v[0], v[1], v[2], v[3]);
    else
      for (int q = 0; q < 4 && i + q < n; ++q) out[i + q] = v[q];
  }
}

// ---- noise-aware masks (noise_aware_IBM / threshold_IBM, target.py:108-251) and the ideal ratio mask, one pass
// A batch of spectra given as interleaved (re, im) pairs, bin (b, t, f) at p[b*sb + t*st + f*sf] (float strides, even).
struct Spec { const float* p; long sb, st, sf; };
struct NaOut { float *speech, *noise, *irm; };

// peak[b]^2 as the divisor of both powers; 1 (no scaling) without a peak or when the square is not finite and positive
__device__ __forceinline__ double peak_sq(const float* __restrict__ peak, int b) {
  if (!peak) return 1.0;
  const double p2 = (double)peak[b] * (double)peak[b];
  return (p2 > 0.0 && p2 < __builtin_huge_val()) ? p2 : 1.0;
}
__device__ __forceinline__ double cell_power(const Spec& s, int b, int t, int f, double p2) {
  const float2 c = *reinterpret_cast<const float2*>(s.p + b * s.sb + t * s.st + f * s.sf);
  return ((double)c.x * c.x + (double)c.y * c.y) / p2;
}

// speech / noise / irm [B][Tp][F] (each may be null): four consecutive outputs per thread, threads along f, so a wave
// reads 2 KB of a spectrum row in a piece and stores one float4 per output; every step in double, thresholds from the
// host's tables c_speech / c_noise (read through the cache: 16 F bytes that every workgroup shares).
__global__ void __launch_bounds__(256)
    noise_aware_mask(Spec X, Spec N, const int* __restrict__ n_frames, const float* __restrict__ peak,
                     const double* __restrict__ c_speech, const double* __restrict__ c_noise, int f_lo, int f_hi, double floor,
                     double noise_psd, int F, int Tp, int B, int vec, NaOut out) {
  const long n = (long)B * Tp * F, n4 = (n + 3) >> 2;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < n4; g += (long)gridDim.x * 256) {
    const long i = g * 4;
    const long m = i / F;
    int f = (int)(i - m * F);
    int b = (int)(m / Tp), t = (int)(m - (long)b * Tp);
    int Tb = row_count(n_frames, b, Tp);
    double p2 = peak_sq(peak, b);
    float vs[4], vn[4], vr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float s = 0.f, z = 0.f, r = 0.f;
      if (i + q < n && t < Tb) {
        const double xP = cell_power(X, b, t, f, p2);
        const double nP = N.p ? cell_power(N, b, t, f, p2) : noise_psd;
        const bool cut = f < f_lo || f >= f_hi;
        const double xs = xP / c_speech[f], xn = xP / c_noise[f];
        s = (!cut && xs > nP && xs > floor) ? 1.f : 0.f;
        z = (cut || xn < nP || xn < floor) ? 1.f : 0.f;
        const double sum = xP + nP;
        r = sum == 0.0 ? 0.f : (float)(xP / sum);
      }
      vs[q] = s, vn[q] = z, vr[q] = r;
      if (++f == F) {                                      // next spectrum row (and maybe the next utterance)
        f = 0;
        if (++t == Tp && i + q + 1 < n) {
          t = 0, ++b;
          Tb = row_count(n_frames, b, Tp);
          p2 = peak_sq(peak, b);
        }
      }
    }
    float* const dst[3] = {out.speech, out.noise, out.irm};
    const float* const src[3] = {vs, vn, vr};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (!dst[k]) continue;
      if ((vec >> k & 1) && i + 3 < n) *reinterpret_cast<float4*>(dst[k] + i) = make_float4(src[k][0], src[k][1], src[k][2], src[k][3]);
      else
        for (int q = 0; q < 4 && i + q < n; ++q) dst[k][i + q] = src[k][q];
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int div_up(long a, long b) { return (int)((a + b - 1) / b); }
inline int grid_cap(long n4, int cap) { const long g = (n4 + 255) / 256; return (int)(g < 1 ? 1 : (g > cap ? cap : g)); }

inline int pad_off(const avvad_target_desc* d) { return d->center ? d->n_fft / 2 : 0; }
// energy segments: hop-sized blocks (R = n_fft / hop of them per frame) when the frame is a whole number of hops
inline int seg_R(const avvad_target_desc* d) { return d->n_fft % d->hop == 0 ? d->n_fft / d->hop : 1; }

bool ok_desc(const avvad_target_desc* d) {
  return d && d->B > 0 && d->B <= 65535 && d->L > 0 && d->n_fft > 0 && d->hop > 0 && d->T > 0 && d->center >= 0 && d->center <= 2 &&
         d->eps >= 0.f && isfinite(d->vad_coef) && d->vad_coef >= 0.0 && isfinite(d->ibm_coef) && d->ibm_coef > 0.0 &&
         (long)d->B * d->T < (1L << 24) &&
         // at most the reference's one-hop end pad behind the longest utterance, plus the centre padding
         (long)(d->T - 1) * d->hop + d->n_fft <= d->L + d->hop + 2L * pad_off(d);
}

struct Layout {                     // workspace carve-up: byte offsets, then the spectrum workspace (float offsets)
  size_t E, vad, maxbits, total;
  frames::SpecWs f;
};
Layout layout(const avvad_target_desc* d) {
  Layout l = {};
  const size_t nseg = (size_t)d->T + seg_R(d) - 1;
  size_t o = 0;
  l.E = o, o += align_up((size_t)d->B * nseg * sizeof(double), 256);
  l.vad = o, o += align_up((size_t)d->B * d->T * sizeof(float), 256);
  l.maxbits = o, o += align_up((size_t)d->B * sizeof(unsigned long long), 256);
  l.total = o;
  if (frames::ok_n_fft(d->n_fft)) { // the DFT GEMM of the waveform IBM
    l.f = frames::spec_ws(d->n_fft, (size_t)d->B * d->T, o / sizeof(float));
    l.total = l.f.total * sizeof(float);
  }
  return l;
}

int vad_impl(const float* wave, const int* n_samples, const int* n_frames, float* vad, const avvad_target_desc* d, char* ws,
             const Layout& l, hipStream_t s) {
  const int R = seg_R(d), nseg = d->T + R - 1;
  const int seg = R > 1 ? d->hop : d->n_fft;
  const int mode = d->center == 1 ? 1 : 0;
  const int vec = aligned16(wave) && d->L % 4 == 0;
  double* E = (double*)(ws + l.E);
  hipLaunchKernelGGL(segment_energy, dim3(div_up(nseg, 4 * SEGS_PER_WAVE), d->B), dim3(256), 0, s, wave, d->L, n_samples, n_frames,
                     d->T, pad_off(d), mode, seg, d->hop, R, nseg, vec, E);
  hipLaunchKernelGGL(vad_decide, dim3(d->B), dim3(256), 0, s, E, nseg, n_frames, R, d->vad_coef, d->T,
                     (int)(aligned16(vad) && d->T % 4 == 0), vad);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

}  // namespace

extern "C" size_t avvad_target_workspace(const avvad_target_desc* d) {
  if (!ok_desc(d)) return 0;
  return layout(d).total;
}

extern "C" int avvad_target_vad(const float* wave, const int* n_samples, const int* n_frames, float* vad, const avvad_target_desc* d,
                                void* ws, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!wave || !n_samples || !n_frames || !vad || !ws || ws_misaligned(ws) || !ok_desc(d)) return AVVAD_EINVAL;
  const Layout l = layout(d);
  if (ws_bytes < l.total) return AVVAD_EWORKSPACE;
  return vad_impl(wave, n_samples, n_frames, vad, d, (char*)ws, l, (hipStream_t)sv);
}

extern "C" int avvad_target_ibm(const float* wave, const int* n_samples, const int* n_frames, int robust, float* ibm,
                                const avvad_target_desc* d, void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!wave || !n_samples || !n_frames || !ibm || !wsv || ws_misaligned(wsv) || !ok_desc(d) || d->center != 0 || !frames::ok_n_fft(d->n_fft))
    return AVVAD_EINVAL;
  const Layout l = layout(d);
  const int ld = l.f.ld, F = d->n_fft / 2 + 1;
  if ((long)d->B * d->T * ld >= (1L << 31)) return AVVAD_EINVAL;
  if (ws_bytes < l.total) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  char* ws = (char*)wsv;
  float* vad = nullptr;
  if (robust) {
    vad = (float*)(ws + l.vad);
    int rc = vad_impl(wave, n_samples, n_frames, vad, d, ws, l, s);
    if (rc) return rc;
  }
  float* S = (float*)ws + l.f.S;
  int rc = frames::framed_dft(wave, d->L, d->B, d->T, d->n_fft, d->hop, (float*)ws, l.f, s);
  if (rc) return rc;
  unsigned long long* maxbits = (unsigned long long*)(ws + l.maxbits);
  if (hipMemsetAsync(maxbits, 0, (size_t)d->B * sizeof(unsigned long long), s) != hipSuccess) return AVVAD_ELAUNCH;
  hipLaunchKernelGGL(spectrum_max, dim3(div_up(d->T, MAX_ROWS), d->B), dim3(256), 0, s, S, ld, d->T, n_frames, maxbits);
  const long n4 = ((long)d->B * d->T * F + 3) / 4;
  hipLaunchKernelGGL(ibm_mask, dim3(grid_cap(n4, 8192)), dim3(256), 0, s, S, ld, F, d->T, d->B, n_frames, maxbits, d->ibm_coef,
                     (double)d->eps, vad, (int)aligned16(ibm), ibm);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

extern "C" int avvad_target_ibm_from_spectrum(const float* spec, long stride_t, long stride_f, const float* vad, float* out,
                                              const avvad_target_desc* d, void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  // only B, n_fft (F = n_fft/2 + 1), T, eps and ibm_coef are read: the spectrum is given, there is no framing
  if (!spec || !out || !wsv || !d || d->B != 1 || d->n_fft < 2 || d->T <= 0 || (long)d->T * (d->n_fft / 2 + 1) >= (1L << 31) ||
      !(d->eps >= 0.f) || !isfinite(d->ibm_coef) || !(d->ibm_coef > 0.0) || stride_t <= 0 || stride_f <= 0 || (stride_t | stride_f) & 1 ||
      ((uintptr_t)spec & 7) || ws_misaligned(wsv))
    return AVVAD_EINVAL;
  if (ws_bytes < sizeof(unsigned long long)) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  const int F = d->n_fft / 2 + 1, T = d->T;
  unsigned long long* maxbits = (unsigned long long*)wsv;
  if (hipMemsetAsync(maxbits, 0, sizeof(unsigned long long), s) != hipSuccess) return AVVAD_ELAUNCH;
  const long n4 = ((long)T * F + 3) / 4;
  hipLaunchKernelGGL(spectrum_max_strided, dim3(grid_cap(n4 * 4, 1024)), dim3(256), 0, s, spec, stride_t, stride_f, T, F, maxbits);
  hipLaunchKernelGGL(ibm_mask_strided, dim3(grid_cap(n4, 4096)), dim3(256), 0, s, spec, stride_t, stride_f, T, F, maxbits,
                     d->ibm_coef, (double)d->eps, vad, (int)aligned16(out), out);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

// ---- noise-aware masks
namespace {

struct NaParams {
  const int* n_frames;
  const float* peak;
  const double *c_speech, *c_noise;
  int low_cut, high_cut;
  double floor, noise_psd;
};
bool ok_na(const NaParams& p, const NaOut& o, int F) {
  return p.c_speech && p.c_noise && !((uintptr_t)p.c_speech & 7) && !((uintptr_t)p.c_noise & 7) && p.low_cut >= 1 &&
         p.high_cut <= F && (o.speech || o.noise || o.irm);
}
bool ok_spec(const Spec& s, int B) {
  return !((uintptr_t)s.p & 7) && s.st > 0 && s.sf > 0 && s.sb >= 0 && (B == 1 || s.sb > 0) && !((s.sb | s.st | s.sf) & 1);
}
int na_launch(const Spec& X, const Spec& N, const NaParams& p, const NaOut& o, int B, int T, int F, hipStream_t s) {
  const long n4 = ((long)B * T * F + 3) / 4;
  const int vec = (int)aligned16(o.speech) | (int)aligned16(o.noise) << 1 | (int)aligned16(o.irm) << 2;
  hipLaunchKernelGGL(noise_aware_mask, dim3(grid_cap(n4, 8192)), dim3(256), 0, s, X, N, p.n_frames, p.peak, p.c_speech, p.c_noise,
                     p.low_cut - 1, p.high_cut, p.floor, p.noise_psd, F, T, B, vec, o);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

// workspace of the waveform entry: [W][S speech][S noise][engine slab] -- one basis and one slab for the two products, which
// run one after the other on the stream; .x / .n are what frames::framed_dft takes for each
struct NaWs { frames::SpecWs x, n; };
NaWs na_ws(const avvad_target_desc* d) {
  NaWs w;
  w.x = frames::spec_ws(d->n_fft, (size_t)d->B * d->T);
  w.n = w.x;
  w.n.S = w.x.S_end;
  w.n.S_end = w.n.S + (w.x.S_end - w.x.S);
  w.n.slab = w.n.S_end;
  w.n.total = w.n.slab + igemm::SLAB_FLOATS;
  w.x.slab = w.n.slab, w.x.total = w.n.total;
  return w;
}
bool ok_na_desc(const avvad_target_desc* d) { return ok_desc(d) && d->center == 0 && frames::ok_n_fft(d->n_fft); }

}  // namespace

extern "C" size_t avvad_target_noise_aware_workspace(const avvad_target_desc* d) {
  if (!ok_na_desc(d)) return 0;
  return na_ws(d).n.total * sizeof(float);
}

extern "C" int avvad_target_noise_aware_from_spectrum(const float* spec, long stride_b, long stride_t, long stride_f,
                                                      const float* noise_spec, long nstride_b, long nstride_t, long nstride_f,
                                                      const int* n_frames, const float* peak, const double* c_speech,
                                                      const double* c_noise, int low_cut, int high_cut, double floor,
                                                      double noise_psd, float* speech, float* noise, float* irm, int B, int T,
                                                      int F, avvad_stream_t sv) {
  AVVAD_ENTER();
  const Spec X = {spec, stride_b, stride_t, stride_f}, N = {noise_spec, nstride_b, nstride_t, nstride_f};
  const NaParams p = {n_frames, peak, c_speech, c_noise, low_cut, high_cut, floor, noise_psd};
  const NaOut o = {speech, noise, irm};
  if (!spec || B <= 0 || T <= 0 || F <= 0 || (long)B * T >= (1L << 31) / F || !ok_na(p, o, F) || !ok_spec(X, B) ||
      (noise_spec && !ok_spec(N, B)))
    return AVVAD_EINVAL;
  return na_launch(X, N, p, o, B, T, F, (hipStream_t)sv);
}

extern "C" int avvad_target_noise_aware(const float* speech_wave, const float* noise_wave, const int* n_samples,
                                        const int* n_frames, const float* peak, const double* c_speech, const double* c_noise,
                                        int low_cut, int high_cut, double floor, float* speech, float* noise, float* irm,
                                        const avvad_target_desc* d, void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  (void)n_samples;                    // rows are zero-padded past each utterance: the DFT reads them as avvad_stft does
  if (!speech_wave || !noise_wave || !n_frames || !wsv || ws_misaligned(wsv) || !ok_na_desc(d)) return AVVAD_EINVAL;
  const int F = d->n_fft / 2 + 1;
  const NaParams p = {n_frames, peak, c_speech, c_noise, low_cut, high_cut, floor, 0.0};
  const NaOut o = {speech, noise, irm};
  const NaWs w = na_ws(d);
  const int ld = w.x.ld;
  if (!ok_na(p, o, F) || (long)d->B * d->T * ld >= (1L << 31)) return AVVAD_EINVAL;
  if (ws_bytes < w.n.total * sizeof(float)) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  float* ws = (float*)wsv;
  // one product per wave with the batch's own (B, T): the stream-K split depends on the row count, and with it the
  // summation order of a bin, so only this gives the bits of avvad_stft_complex for the same batch
  int rc = frames::framed_dft(speech_wave, d->L, d->B, d->T, d->n_fft, d->hop, ws, w.x, s);
  if (rc) return rc;
  rc = frames::framed_dft(noise_wave, d->L, d->B, d->T, d->n_fft, d->hop, ws, w.n, s);
  if (rc) return rc;
  const Spec X = {ws + w.x.S, (long)d->T * ld, ld, 2}, N = {ws + w.n.S, (long)d->T * ld, ld, 2};
  return na_launch(X, N, p, o, d->B, d->T, F, s);
}
