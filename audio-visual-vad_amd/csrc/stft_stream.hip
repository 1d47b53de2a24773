// stft_stream.hip -- the STFT front-end on a stream of samples: each row carries the samples that did not yet complete a
// frame (or that later frames still overlap) across calls, and a call emits the log-power (optionally standardised)
// features of exactly the frames its new samples complete.  One launch per call: framing, peak division, windowed real
// DFT on fp32 MFMA, |X|^2 -> log -> standardisation, the new tail.  avvad_stft_stream_fwd_spec is the same launch with the
// complex spectrum stored beside the features (what the streaming inverse, istft_stream.hip, takes).
//
// The shape is M = a few frames (1 .. a few hundred) against K = n_fft, N = 2 (n_fft/2 + 1): a basis-streaming product, not
// a tile GEMM.  Workgroup blockIdx.x owns 16 bins; it reads its slab of the basis (2 x 16 x K floats, packed so that a
// wave's operand load is 1 KiB contiguous) once per pass of 16 NG frames, which sit in LDS.  Real and imaginary parts of
// a bin are two MFMA accumulators of the same lane, so re^2 + im^2 never leaves it.
//
// SUMMATION ORDER.  One output value is always summed the same way, whatever M, the row, the frame's place in the call or
// the number of pending samples: wave w of 8 accumulates the 16-sample groups kk = w, w + 8, ... of its K-slice in that
// order (an MFMA column does not see the other columns), and the 8 partial sums are added in wave order.  Nothing else
// enters: no atomics, no second kernel form above a size.
#include "frames.h"

namespace {

constexpr int SS_NT = 512;          // threads per workgroup: 8 waves over K
constexpr int SS_NW = SS_NT / 64;
constexpr int SS_PAD = 4;           // frame pitch K + 4 floats: the 16 frames of a ds_read_b128 lane group sit on 16 different slots
constexpr size_t SS_LDS_MAX = 150 * 1024;

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

// k index that lane-quarter q reads in MFMA j of sample group kk: both operands use it, so the product is a plain sum over k
__device__ __forceinline__ int ss_k(int K, int kk, int q, int j) { return (K >> 2) * q + 4 * kk + j; }

// packed basis: [bin block][re, im][kk][lane][4]; value = hann[k] cos(2 pi f k / N) / -hann[k] sin(2 pi f k / N); bins >= F
// are zero
__global__ void ss_basis_kernel(float* __restrict__ W, int N, int F, long n) {
  const int KQ = N >> 4;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
    const int j = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    const long r = idx >> 8;
    const int kk = (int)(r % KQ);
    const int c = (int)((r / KQ) & 1), nb = (int)(r / KQ / 2);
    const int k = ss_k(N, kk, lane >> 4, j), f = 16 * nb + (lane & 15);
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
  int nv = a.n_valid[b], np = a.n_pending[b], nf = a.n_frames[b];
  r.nv = nv < 0 ? 0 : (nv > a.L ? a.L : nv);
  r.np = np < 0 ? 0 : (np > a.K ? a.K : np);
  const int Ls = r.nv + r.np;
  int cap = (Ls >= a.K ? (Ls - a.K) / a.hop + 1 : 0) + (a.pad_frames[b] ? 1 : 0);   // only a row that ends may read past its end
  if (cap > a.T) cap = a.T;
  r.nf = nf < 0 ? 0 : (nf > cap ? cap : nf);
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
__global__ void __launch_bounds__(SS_NT) ss_fwd_kernel(const SsArgs a) {
  // All LDS is the dynamic region, so that its base is offset 0 and every 16-byte access below is aligned: frames
  // [16 NG][K + 4], afterwards the waves' partial sums; behind them (a.tab floats in) the pass's per-frame tables.
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int FP = 16 * NG;
  int* fb = reinterpret_cast<int*>(lds + a.tab);          // per frame of the pass: row, frame of the row, the row's counts
  int *ft = fb + FP, *fnp = ft + FP, *fnv = fnp + FP;
  float* fpk = reinterpret_cast<float*>(fnv + FP);
  int& shM = *reinterpret_cast<int*>(fpk + FP);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int K = a.K, P = K + SS_PAD, KQ = K >> 4, nb = blockIdx.x;
  const float4* wre = reinterpret_cast<const float4*>(a.basis) + ((long)(nb * 2) * KQ) * 64 + lane;
  const float4* wim = wre + (long)KQ * 64;

  for (int pass = blockIdx.y;; pass += gridDim.y) {
    const int m0 = pass * FP;
    if (wave == 0) {       // frame m of the call -> (row, frame of the row): running sum of the rows' frame counts
      int base = 0;
      for (int c0 = 0; c0 < a.B; c0 += 64) {
        const int b = c0 + lane;
        SsRow r{0, 0, 0};
        if (b < a.B) r = ss_row(a, b);
        const int nf = r.nf;
        const float pk = b < a.B && a.peak ? a.peak[b] : 1.f;
        int incl = nf;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(incl, o, 64);
          if (lane >= o) incl += t;
        }
        const int excl = base + incl - nf;
        const int lo = excl > m0 ? excl : m0, hi = excl + nf < m0 + FP ? excl + nf : m0 + FP;
        for (int m = lo; m < hi; ++m) {
          fb[m - m0] = b;
          ft[m - m0] = m - excl;
          fnp[m - m0] = r.np;
          fnv[m - m0] = r.nv;
          fpk[m - m0] = pk;
        }
        base += __shfl(incl, 63, 64);
      }
      if (lane == 0) shM = base;
    }
    __syncthreads();
    const int M = shM;
    if (m0 >= M) break;                          // uniform
    const int nfp = M - m0 < FP ? M - m0 : FP;   // frames of this pass
    // ---- stage the frames, divided by the row's peak (a division, so that a peak of 1 changes no bit)
    // (wave w takes frames w, w + 8, ...: a frame's row, offset and peak are read once, the sample loads are independent)
    for (int fr = wave; fr < nfp; fr += SS_NW) {
      const int b = fb[fr];
      const SsRow r{fnv[fr], fnp[fr], 0};
      const long s0 = (long)ft[fr] * a.hop;
      const float pk = fpk[fr];
      float* dst = lds + fr * P;
#pragma unroll 8
      for (int k = lane; k < K; k += 64) dst[k] = ss_sample(a, b, r, s0 + k) / pk;
    }
    __syncthreads();
    // ---- the product: this wave's sample groups of the slab against the pass's frames
    f32x4 are[NG], aim[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) are[g] = aim[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* frow = lds + i * P + (K >> 2) * q;
    for (int kk = wave; kk < KQ; kk += SS_NW) {
      const float4 cr = wre[(long)kk * 64], ci = wim[(long)kk * 64];
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        if (16 * g < nfp) {                      // uniform
          const float4 x = *reinterpret_cast<const float4*>(frow + 16 * g * P + 4 * kk);
          are[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(cr.x, x.x, are[g], 0, 0, 0);
          aim[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ci.x, x.x, aim[g], 0, 0, 0);
          are[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(cr.y, x.y, are[g], 0, 0, 0);
          aim[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ci.y, x.y, aim[g], 0, 0, 0);
          are[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(cr.z, x.z, are[g], 0, 0, 0);
          aim[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ci.z, x.z, aim[g], 0, 0, 0);
          are[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(cr.w, x.w, are[g], 0, 0, 0);
          aim[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ci.w, x.w, aim[g], 0, 0, 0);
        }
      }
    }
    __syncthreads();                             // every wave has read the frames: the space now takes the partial sums
    f32x4* part = reinterpret_cast<f32x4*>(lds); // [NG][2][8 waves][64 lanes]
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      part[((g * 2 + 0) * SS_NW + wave) * 64 + lane] = are[g];
      part[((g * 2 + 1) * SS_NW + wave) * 64 + lane] = aim[g];
    }
    __syncthreads();
    // ---- wave w finishes register r = w & 3 (bin 4 q + r of the block) of frame group w >> 2: the eight partial sums in
    // wave order, then the epilogue in the lane
    const int g = wave >> 2, r = wave & 3;
    if (g < NG && 16 * g + i < nfp) {
      const float* pf = reinterpret_cast<const float*>(part);
      float re = pf[(((g * 2 + 0) * SS_NW) * 64 + lane) * 4 + r], im = pf[(((g * 2 + 1) * SS_NW) * 64 + lane) * 4 + r];
      for (int w = 1; w < SS_NW; ++w) {
        re += pf[(((g * 2 + 0) * SS_NW + w) * 64 + lane) * 4 + r];
        im += pf[(((g * 2 + 1) * SS_NW + w) * 64 + lane) * 4 + r];
      }
      const int fr = 16 * g + i, f = 16 * nb + 4 * q + r;
      if (f < a.F) {
        float v = logf(fmaf(re, re, im * im) + a.eps);
        if (a.mean) v = (v - a.mean[f]) / (a.stdv[f] + a.norm_eps);
        a.out[((long)fb[fr] * a.T + ft[fr]) * a.F + f] = v;
        if constexpr (SPEC) *reinterpret_cast<float2*>(a.spec + (((long)fb[fr] * a.T + ft[fr]) * a.F + f) * 2) = float2{re, im};
      }
    }
    __syncthreads();                             // the partial sums are read before the next pass stages over them
  }

  // ---- frames a row does not fill are zero (this block's bins), shared out over the grid's second dimension
  const int f0 = 16 * nb, fw = a.F - f0 < 16 ? a.F - f0 : 16;
  for (int b = blockIdx.y * (SS_NT / 16) + (tid >> 4); b < a.B; b += gridDim.y * (SS_NT / 16)) {   // 16 lanes per row
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
      for (int k = tid; k < K; k += SS_NT) so[k] = si[k];
      continue;
    }
    const long start = (long)r.nf * a.hop;
    long len = (long)r.np + r.nv - start;
    len = len < 0 ? 0 : (len > K ? K : len);
    for (int k = tid; k < K; k += SS_NT) so[k] = k < len ? ss_sample(a, b, r, start + k) : 0.f;
  }
}

bool ss_desc_ok(const avvad_stft_stream_desc* d) {
  return d && d->B > 0 && d->L >= 1 && frames::ok_n_fft(d->n_fft) && d->hop >= 1 && d->hop <= d->n_fft && d->T >= 0 &&
         d->M >= 0 && (long)d->T * d->hop < (1L << 30) && (long)d->B * d->L < (1L << 40) &&
         (long)d->B * d->T < (1L << 31) - 64;
}
size_t ss_lds_bytes(int K, int NG) {
  const size_t frames = (size_t)16 * NG * (K + SS_PAD) * sizeof(float), parts = (size_t)NG * 2 * SS_NW * 64 * sizeof(f32x4);
  return frames > parts ? frames : parts;      // both multiples of 16 bytes
}
size_t ss_tab_bytes(int NG) { return align_up((size_t)(5 * 16 * NG + 1) * sizeof(float), 16); }
inline int ss_bin_blocks(int n_fft) { return (n_fft / 2 + 1 + 15) / 16; }

template <int NG, bool SPEC>
int ss_launch(const SsArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  if (int rc = allow_large_lds<ss_fwd_kernel<NG, SPEC>>(lds, SS_LDS_MAX)) return rc;
  hipLaunchKernelGGL((ss_fwd_kernel<NG, SPEC>), grid, dim3(SS_NT), lds, s, a);
  return AVVAD_OK;
}

template <bool SPEC>
int ss_forward(const float* chunk, const int* n_valid, const int* n_pending, const int* n_frames, const int* pad_frames,
               const float* peak, const float* state_in, float* state_out, const float* basis, const float* mean,
               const float* stdv, float* out, float* spec, const avvad_stft_stream_desc* d, hipStream_t s) {
  if (!chunk || !n_valid || !n_pending || !n_frames || !pad_frames || !state_in || !state_out || !basis || !ss_desc_ok(d) ||
      state_in == state_out || (d->T > 0 && !out) || (SPEC && ((d->T > 0 && !spec) || ((uintptr_t)spec & 7))) || !mean != !stdv || ws_misaligned(basis))
    return AVVAD_EINVAL;
  const int K = d->n_fft;
  const long hint = d->M > 0 ? d->M : (long)d->B * d->T;
  int NG = hint > 16 ? 2 : 1;
  if (NG == 2 && ss_lds_bytes(K, 2) + ss_tab_bytes(2) > SS_LDS_MAX) NG = 1;
  if (ss_lds_bytes(K, NG) + ss_tab_bytes(NG) > SS_LDS_MAX) return AVVAD_EINVAL;
  long ny = (hint + 16 * NG - 1) / (16 * NG);
  ny = ny < 1 ? 1 : (ny > 16 ? 16 : ny);         // the passes beyond walk the grid's second dimension
  SsArgs a{chunk, n_valid, n_pending, n_frames, pad_frames, peak, state_in, state_out, basis, mean, stdv, out,
           d->B, d->L, K, d->hop, d->T, K / 2 + 1, (int)(ss_lds_bytes(K, NG) / sizeof(float)), d->eps, d->norm_eps, spec};
  const dim3 grid(ss_bin_blocks(K), (int)ny);
  const int rc = NG == 2 ? ss_launch<2, SPEC>(a, grid, ss_lds_bytes(K, 2) + ss_tab_bytes(2), s)
                         : ss_launch<1, SPEC>(a, grid, ss_lds_bytes(K, 1) + ss_tab_bytes(1), s);
  if (rc) return rc;
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

}  // namespace

extern "C" size_t avvad_stft_stream_basis_bytes(int n_fft) {
  if (!frames::ok_n_fft(n_fft)) return 0;
  return (size_t)ss_bin_blocks(n_fft) * 2 * 16 * n_fft * sizeof(float);
}

extern "C" int avvad_stft_stream_basis(int n_fft, float* out, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!out || !frames::ok_n_fft(n_fft) || ((uintptr_t)out & 15)) return AVVAD_EINVAL;
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
