// stft_stream.hip -- the STFT front-end on a stream of samples: each row carries the samples that did not yet complete a
// frame (or that later frames still overlap) across calls, and a call emits the log-power (optionally standardised)
// features of exactly the frames its new samples complete.  One launch per call: framing, peak division, windowed real
// DFT on fp32 MFMA, |X|^2 -> log -> standardisation, the new tail.  avvad_stft_stream_fwd_spec is the same launch with the
// complex spectrum stored beside the features (what the streaming inverse, istft_stream.hip, takes).
//
// The transform is the basis-streaming product of stream_product.h: K = n_fft against the two planes (re, im) of the 16 bins
// that workgroup blockIdx.x owns, summed in the order that header fixes (SUMMATION ORDER).  Real and imaginary parts of a
// bin are two MFMA accumulators of the same lane, so re^2 + im^2 never leaves it.  This file's own: a row's counts and
// logical stream, staging with the peak division, the log-power / standardise epilogue, the zero fill and the new tail.
#include "stream_product.h"

namespace {

namespace sp = sprod;

constexpr int SS_SLOT_INTS = 5;   // per frame slot of a pass: row, frame of the row, the row's pending and valid counts, its peak

struct SsArgs {
  const float* chunk;
  const int *n_valid, *n_pending, *n_frames, *pad_frames;
  const float *peak, *state_in;
  float* state_out;
  const float *basis, *mean, *stdv;
  float* out;
  int B, L, K, hop, T, F;
  int tab;                  // float offset of the per-frame tables in LDS (behind the frames / partial sums)
  float eps, norm_eps;
  float* spec;              // [B][T][F][2] (re, im) of the same frames: only the SPEC instantiations read it
};

// packed basis: [bin block][re, im][kk][lane][4]; value = hann[k] cos(2 pi f k / N) / -hann[k] sin(2 pi f k / N); bins >= F
// are zero
__global__ void ss_basis_kernel(float* __restrict__ W, int N, int F, long n) {
  const int KQ = N >> 4;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
    const int j = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    const long r = idx >> 8;
    const int kk = (int)(r % KQ);
    const int c = (int)((r / KQ) & 1), nb = (int)(r / KQ / 2);
    const int k = sp::operand_index(N, kk, lane >> 4, j), f = 16 * nb + (lane & 15);
    float v = 0.f;
    if (f < F) {
      const double win = frames::hann(k, N);
      const frames::Phase ph = frames::phase(f, k, N);
      v = (float)(c ? -win * ph.sin() : win * ph.cos());
    }
    W[idx] = v;
  }
}

struct SsRow { int nv, np, nf; };
// the counts of row b as the kernel uses them: everything clamped, so that inconsistent counts cannot reach outside a buffer
__device__ __forceinline__ SsRow ss_row(const SsArgs& a, int b) {
  SsRow r;
  const int nf = a.n_frames[b];
  r.nv = clamp_count(a.n_valid[b], a.L);
  r.np = clamp_count(a.n_pending[b], a.K);
  const int Ls = r.nv + r.np;
  int cap = (Ls >= a.K ? (Ls - a.K) / a.hop + 1 : 0) + (a.pad_frames[b] ? 1 : 0);   // only a row that ends may read past its end
  if (cap > a.T) cap = a.T;
  r.nf = clamp_count(nf, cap);
  return r;
}
// sample s of row b's logical stream (pending tail, then the chunk; zero past the end)
__device__ __forceinline__ float ss_sample(const SsArgs& a, int b, const SsRow& r, long s) {
  if (s < r.np) return a.state_in[(long)b * a.K + s];
  s -= r.np;
  return s < r.nv ? a.chunk[(long)b * a.L + s] : 0.f;
}

// SPEC: the epilogue also stores (re, im), the complex spectrum of the samples / peak, for the streaming inverse
// (istft_stream.hip).  A template parameter, so that the instantiations behind avvad_stft_stream_fwd stay what they were.
template <int NG, bool SPEC>
__global__ void __launch_bounds__(sp::NT) ss_fwd_kernel(const SsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int FP = 16 * NG;
  const sp::Tables<FP, SS_SLOT_INTS> tb(lds + a.tab);
  int *fnp = tb.own(0), *fnv = tb.own(1);
  float* fpk = reinterpret_cast<float*>(tb.own(2));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int K = a.K, P = K + sp::PAD, nb = blockIdx.x;
  const f32x4* wb = reinterpret_cast<const f32x4*>(a.basis) + ((long)(nb * 2) * (K >> 4)) * 64 + lane;

  for (int pass = blockIdx.y;; pass += gridDim.y) {
    SsRow row;
    float peak;
    const int nfp = sp::map_frames(
        tb, a.B, pass * FP,
        [&](int b) {
          row = ss_row(a, b);
          peak = a.peak ? a.peak[b] : 1.f;
          return row.nf;
        },
        [&](int slot) {
          fnp[slot] = row.np;
          fnv[slot] = row.nv;
          fpk[slot] = peak;
        });
    if (nfp <= 0) break;                         // uniform
    // ---- stage the frames, divided by the row's peak (a division, so that a peak of 1 changes no bit)
    // (wave w takes frames w, w + 8, ...: a frame's row, offset and peak are read once, the sample loads are independent)
    for (int fr = wave; fr < nfp; fr += sp::NW) {
      const int b = tb.fb[fr];
      const SsRow r{fnv[fr], fnp[fr], 0};
      const long s0 = (long)tb.ft[fr] * a.hop;
      const float pk = fpk[fr];
      float* dst = lds + fr * P;
#pragma unroll 8
      for (int k = lane; k < K; k += 64) dst[k] = ss_sample(a, b, r, s0 + k) / pk;
    }
    __syncthreads();
    sp::product<NG, 2>(lds, wb, K, nfp);
    // ---- wave w finishes register r = w & 3 (bin 4 q + r of the block) of frame group w >> 2, then the epilogue in the lane
    const int g = wave >> 2, r = wave & 3;
    if (g < NG && 16 * g + i < nfp) {
      const float re = sp::finish<2>(lds, g, 0, lane, r), im = sp::finish<2>(lds, g, 1, lane, r);
      const int fr = 16 * g + i, f = 16 * nb + 4 * q + r;
      if (f < a.F) {
        const long o = ((long)tb.fb[fr] * a.T + tb.ft[fr]) * a.F + f;
        float v = logf(fmaf(re, re, im * im) + a.eps);
        if (a.mean) v = (v - a.mean[f]) / (a.stdv[f] + a.norm_eps);
        a.out[o] = v;
        if constexpr (SPEC) *reinterpret_cast<float2*>(a.spec + o * 2) = float2{re, im};
      }
    }
    __syncthreads();                             // the partial sums are read before the next pass stages over them
  }

  // ---- frames a row does not fill are zero (this block's bins), shared out over the grid's second dimension
  const int f0 = 16 * nb, fw = a.F - f0 < 16 ? a.F - f0 : 16;
  for (int b = blockIdx.y * (sp::NT / 16) + (tid >> 4); b < a.B; b += gridDim.y * (sp::NT / 16)) {   // 16 lanes per row
    const int nf = ss_row(a, b).nf;
    if ((tid & 15) < fw)
      for (int t = nf; t < a.T; ++t) {
        a.out[((long)b * a.T + t) * a.F + f0 + (tid & 15)] = 0.f;
        if constexpr (SPEC) *reinterpret_cast<float2*>(a.spec + (((long)b * a.T + t) * a.F + f0 + (tid & 15)) * 2) = float2{0.f, 0.f};
      }
  }
  // ---- the new tail of the rows this workgroup looks after: the stream from the start of the next frame on
  for (int b = blockIdx.y * gridDim.x + nb; b < a.B; b += gridDim.x * gridDim.y) {
    const SsRow r = ss_row(a, b);
    const float* si = a.state_in + (long)b * K;
    float* so = a.state_out + (long)b * K;
    if (a.n_valid[b] <= 0 && r.nf == 0) {        // idle row: bit for bit
      for (int k = tid; k < K; k += sp::NT) so[k] = si[k];
      continue;
    }
    const long start = (long)r.nf * a.hop;
    long len = (long)r.np + r.nv - start;
    len = len < 0 ? 0 : (len > K ? K : len);
    for (int k = tid; k < K; k += sp::NT) so[k] = k < len ? ss_sample(a, b, r, start + k) : 0.f;
  }
}

bool ss_desc_ok(const avvad_stft_stream_desc* d) {
  return d && d->B > 0 && d->L >= 1 && frames::ok_n_fft(d->n_fft) && d->n_fft <= sp::K_MAX && d->hop >= 1 && d->hop <= d->n_fft && d->T >= 0 &&
         d->M >= 0 && (long)d->T * d->hop < (1L << 30) && (long)d->B * d->L < (1L << 40) &&
         (long)d->B * d->T < (1L << 31) - 64;
}
inline int ss_bin_blocks(int n_fft) { return (n_fft / 2 + 1 + 15) / 16; }

template <bool SPEC>
int ss_forward(const float* chunk, const int* n_valid, const int* n_pending, const int* n_frames, const int* pad_frames,
               const float* peak, const float* state_in, float* state_out, const float* basis, const float* mean,
               const float* stdv, float* out, float* spec, const avvad_stft_stream_desc* d, hipStream_t s) {
  if (!chunk || !n_valid || !n_pending || !n_frames || !pad_frames || !state_in || !state_out || !basis || !ss_desc_ok(d) ||
      state_in == state_out || (d->T > 0 && !out) || (SPEC && ((d->T > 0 && !spec) || ((uintptr_t)spec & 7))) || !mean != !stdv || ws_misaligned(basis))
    return AVVAD_EINVAL;
  const int K = d->n_fft;
  const sp::Plan p = sp::plan(K, 2, SS_SLOT_INTS, d->M > 0 ? d->M : (long)d->B * d->T);
  if (!p.NG) return AVVAD_EINVAL;
  SsArgs a{chunk, n_valid, n_pending, n_frames, pad_frames, peak, state_in, state_out, basis, mean, stdv, out,
           d->B, d->L, K, d->hop, d->T, K / 2 + 1, p.tab, d->eps, d->norm_eps, spec};
  const dim3 grid(ss_bin_blocks(K), p.ny);
  const int rc = p.NG == 2 ? sp::launch<ss_fwd_kernel<2, SPEC>>(a, grid, p.lds, s)
                           : sp::launch<ss_fwd_kernel<1, SPEC>>(a, grid, p.lds, s);
  if (rc) return rc;
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

}  // namespace

extern "C" size_t avvad_stft_stream_basis_bytes(int n_fft) {
  if (!frames::ok_n_fft(n_fft) || n_fft > sp::K_MAX) return 0;
  return (size_t)ss_bin_blocks(n_fft) * 2 * 16 * n_fft * sizeof(float);
}

extern "C" int avvad_stft_stream_basis(int n_fft, float* out, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!out || !avvad_stft_stream_basis_bytes(n_fft) || ((uintptr_t)out & 15)) return AVVAD_EINVAL;
  const long n = (long)(avvad_stft_stream_basis_bytes(n_fft) / sizeof(float));
  hipLaunchKernelGGL(ss_basis_kernel, dim3(frames::grid1(n)), dim3(256), 0, (hipStream_t)sv, out, n_fft, n_fft / 2 + 1, n);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

extern "C" int avvad_stft_stream_fwd(const float* chunk, const int* n_valid, const int* n_pending, const int* n_frames,
                                     const int* pad_frames, const float* peak, const float* state_in, float* state_out,
                                     const float* basis, const float* mean, const float* stdv, float* out,
                                     const avvad_stft_stream_desc* d, avvad_stream_t sv) {
  AVVAD_ENTER();
  return ss_forward<false>(chunk, n_valid, n_pending, n_frames, pad_frames, peak, state_in, state_out, basis, mean, stdv, out,
                           nullptr, d, (hipStream_t)sv);
}

extern "C" int avvad_stft_stream_fwd_spec(const float* chunk, const int* n_valid, const int* n_pending, const int* n_frames,
                                          const int* pad_frames, const float* peak, const float* state_in, float* state_out,
                                          const float* basis, const float* mean, const float* stdv, float* out, float* spec,
                                          const avvad_stft_stream_desc* d, avvad_stream_t sv) {
  AVVAD_ENTER();
  return ss_forward<true>(chunk, n_valid, n_pending, n_frames, pad_frames, peak, state_in, state_out, basis, mean, stdv, out,
                          spec, d, (hipStream_t)sv);
}
