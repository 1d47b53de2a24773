// istft_stream.hip -- the masked inverse STFT on a stream of frames: the mirror of stft_stream.hip.  A call takes the next
// few frames of every row's spectrum (as avvad_stft_stream_fwd_spec hands them out) and a mask, and emits the samples that
// no later frame can cover any more; each row's unfinished overlap-add sums travel from call to call in a [B][n_fft] state.
//
// Two launches.  (1) The product Y[(b,t)][n] = sum_c A[(b,t)][c] Winv[c][n]: M = a handful of frames against K = N = n_fft,
// so a basis-streaming fp32-MFMA product like the forward's, not a tile GEMM.  Workgroup blockIdx.x owns 16 output-sample
// columns n; it reads its slab of the basis (16 x K floats, packed so that a wave's operand load is 1 KiB contiguous) once per
// pass of 16 NG frames, which sit in LDS with the mask multiplied in while they are staged -- the masked spectrum never exists
// in memory.  (2) The overlap-add: one thread per output sample and per state element.  One frame's 16 columns overlap-add
// into other workgroups' columns unless hop divides n_fft, and a fusion in which a workgroup owned a residue class of
// samples would leave hop / 16 workgroups; hence the second launch.
//
// REAL-FFT PACKING.  The inverse of a half spectrum ignores im[0] and im[n_fft/2], so the contraction is packed to exactly
// K = n_fft rows: c = 0 is re[0], c = 1 is re[n_fft/2], c = 2f, 2f + 1 are re[f], im[f] for 1 <= f < n_fft/2.  K is then a
// multiple of 32 like the forward's, not n_fft + 2.
//
// SUMMATION ORDER.  Y[(b,t)][n] is always summed the same way, whatever M, the row or the frame's place in the call: wave w
// of 8 accumulates the groups kk = w, w + 8, ... of its K-slice in that order and the 8 partial sums are added in wave order.
// An output sample is the chain state + Y[b,0] + Y[b,1] + ... in ascending frame order; the state is that chain cut at the
// call boundary, and it starts at +0.  So the sum of one sample is the whole-utterance chain of overlap_add (istft.hip)
// for every split of a stream into calls: the same bits.  No atomics, no second kernel form above a size.
#include "frames.h"

namespace {

constexpr int IS_NT = 512;          // threads per workgroup: 8 waves over K
constexpr int IS_NW = IS_NT / 64;
constexpr int IS_PAD = 4;           // frame pitch K + 4 floats, as in the forward
constexpr size_t IS_LDS_MAX = 150 * 1024;
constexpr float IS_F32_TINY = 1.17549435e-38f;
constexpr int IS_E0_MAX = 1 << 30;  // frames a row may have behind it

struct IsArgs {
  const float *spec, *mask;
  const int* n_frames;
  const float* basis;
  float* Y;
  int B, T, K, F, mode;
  int tab;                  // float offset of the per-frame tables in LDS
};

// contraction index that lane-quarter q reads in MFMA j of group kk (the forward's rule)
__device__ __forceinline__ int is_c(int K, int kk, int q, int j) { return (K >> 2) * q + 4 * kk + j; }

__device__ __forceinline__ int is_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// packed basis [column block][kk][lane][4]: element (c, n) of the windowed inverse real DFT, c the packed contraction row;
// behind it hann^2 as n_fft doubles
__global__ void is_basis_kernel(float* __restrict__ W, double* __restrict__ win2, int N, long n_el) {
  const int KQ = N >> 4;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n_el; idx += (long)gridDim.x * blockDim.x) {
    const int j = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    const long r = idx >> 8;
    const int kk = (int)(r % KQ), nb = (int)(r / KQ);
    const int c = is_c(N, kk, lane >> 4, j), n = 16 * nb + (lane & 15);
    const int f = c == 0 ? 0 : (c == 1 ? N / 2 : c >> 1);
    const bool imag = c >= 2 && (c & 1);
    const double win = frames::hann(n, N);
    const double wf = (f == 0 || 2 * f == N) ? 1.0 : 2.0;
    const frames::Phase ph = frames::phase(f, n, N);
    W[idx] = (float)(imag ? -win * (wf / (double)N) * ph.sin() : win * (wf / (double)N) * ph.cos());
    if (idx < N) {
      const double w = frames::hann((int)idx, N);
      win2[idx] = w * w;
    }
  }
}

// SIG: the mask is sigmoid(logit) (mode 2; its own instantiation, as in istft.hip)
template <int NG, bool SIG>
__global__ void __launch_bounds__(IS_NT) is_product_kernel(const IsArgs a) {
  // All LDS is the dynamic region (base offset 0, every 16-byte access aligned): frames [16 NG][K + 4], afterwards the
  // waves' partial sums; behind them (a.tab floats in) the pass's per-frame tables.
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int FP = 16 * NG;
  int* fb = reinterpret_cast<int*>(lds + a.tab);          // per frame of the pass: row, frame of the row
  int* ft = fb + FP;
  int& shM = *(ft + FP);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int K = a.K, P = K + IS_PAD, KQ = K >> 4, nb = blockIdx.x;
  const float4* wb = reinterpret_cast<const float4*>(a.basis) + ((long)nb * KQ) * 64 + lane;

  for (int pass = blockIdx.y;; pass += gridDim.y) {
    const int m0 = pass * FP;
    if (wave == 0) {       // frame m of the call -> (row, frame of the row): running sum of the rows' frame counts
      int base = 0;
      for (int c0 = 0; c0 < a.B; c0 += 64) {
        const int b = c0 + lane;
        const int nf = b < a.B ? is_clamp(a.n_frames[b], a.T) : 0;
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
        }
        base += __shfl(incl, 63, 64);
      }
      if (lane == 0) shM = base;
    }
    __syncthreads();
    const int M = shM;
    if (m0 >= M) break;                          // uniform
    const int nfp = M - m0 < FP ? M - m0 : FP;   // frames of this pass
    // ---- stage the frames in the packed order, times the mask (wave w takes frames w, w + 8, ...).  Frame rows of a
    // 16-frame group that the pass does not fill keep what LDS held: an MFMA column does not see the other columns, and
    // theirs is never stored.
    for (int fr = wave; fr < nfp; fr += IS_NW) {
      float* dst = lds + fr * P;
      const long m = (long)fb[fr] * a.T + ft[fr];
      const float* src = a.spec + m * a.F * 2;
      const float* mk = a.mask + m * a.F;
#pragma unroll 4
      for (int c = lane; c < K; c += 64) {
        const int f = c == 0 ? 0 : (c == 1 ? K >> 1 : c >> 1);
        float v = src[c == 1 ? K : c];           // (re, im) adjacent: re[f] at 2f, im[f] at 2f + 1
        if (a.mode) {
          const float g = mk[f];
          if constexpr (SIG) v *= 1.f / (1.f + expf(-g));
          else v *= a.mode == 1 ? g : (g > 0.f ? 1.f : 0.f);
        }
        dst[c] = v;
      }
    }
    __syncthreads();
    // ---- the product: this wave's groups of the slab against the pass's frames
    f32x4 acc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* frow = lds + i * P + (K >> 2) * q;
    for (int kk = wave; kk < KQ; kk += IS_NW) {
      const float4 w = wb[(long)kk * 64];
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        if (16 * g < nfp) {                      // uniform
          const float4 x = *reinterpret_cast<const float4*>(frow + 16 * g * P + 4 * kk);
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, x.x, acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, x.y, acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, x.z, acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, x.w, acc[g], 0, 0, 0);
        }
      }
    }
    __syncthreads();                             // every wave has read the frames: the space now takes the partial sums
    f32x4* part = reinterpret_cast<f32x4*>(lds); // [NG][8 waves][64 lanes]: register r of lane (i, q) is column 4 q + r of frame i
#pragma unroll
    for (int g = 0; g < NG; ++g) part[(g * IS_NW + wave) * 64 + lane] = acc[g];
    __syncthreads();
    // ---- thread (frame, column): the eight partial sums in wave order, 16 columns of a frame as one 64-byte store
    const int fr = tid >> 4, col = tid & 15;
    if (fr < nfp) {
      const float* pf = reinterpret_cast<const float*>(part);
      const int g = fr >> 4, src = ((fr & 15) + 16 * (col >> 2)) * 4 + (col & 3);
      float y = pf[(g * IS_NW) * 256 + src];
      for (int w = 1; w < IS_NW; ++w) y += pf[(g * IS_NW + w) * 256 + src];
      a.Y[((long)fb[fr] * a.T + ft[fr]) * K + 16 * nb + col] = y;
    }
    __syncthreads();                             // the partial sums are read before the next pass stages over them
  }
}

struct OlaArgs {
  const float* Y;
  const double* win2;
  const int *n_frames, *n_before, *n_out;
  const float *scale, *state_in;
  float *state_out, *out;
  int B, T, N, hop, L;
};

// call-relative sample p of row b: the chain state + Y[b,i][p - i hop] over the call's frames i that cover it, ascending
__device__ __forceinline__ float ola_sum(const OlaArgs& a, int b, int nf, long p) {
  float acc = p < a.N ? a.state_in[(long)b * a.N + p] : 0.f;
  const long lo = p - a.N + 1;
  const int i0 = lo > 0 ? (int)((lo + a.hop - 1) / a.hop) : 0;
  long i1 = p / a.hop;
  if (i1 > nf - 1) i1 = nf - 1;
  for (int i = i0; i <= (int)i1; ++i) acc += a.Y[((long)b * a.T + i) * a.N + (int)(p - (long)i * a.hop)];
  return acc;
}

// One thread per element of out [B][L] and of state_out [B][N].  Every count is clamped, so that inconsistent counts
// cannot reach outside a buffer.  A row whose n_out differs from n_frames * hop ends with this call (a final flush):
// what it does not emit is dropped and its new state is all zero.
__global__ void is_ola_kernel(const OlaArgs a) {
  const int pitch = a.L + a.N;
  const long n_el = (long)a.B * pitch;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n_el; idx += (long)gridDim.x * blockDim.x) {
    const int b = (int)(idx / pitch), p = (int)(idx % pitch);
    const int nf = is_clamp(a.n_frames[b], a.T), e0 = is_clamp(a.n_before[b], IS_E0_MAX), no = is_clamp(a.n_out[b], a.L);
    const long adv = (long)nf * a.hop;
    if (p >= a.L) {                              // ---- state element q: the partial sum of call sample nf hop + q
      const int qs = p - a.L;
      float v;
      if (nf == 0 && no == 0) v = a.state_in[(long)b * a.N + qs];   // idle row: bit for bit
      else if ((long)no != adv) v = 0.f;                              // the row ends here
      else v = qs < a.N - a.hop ? ola_sum(a, b, nf, adv + qs) : 0.f;
      a.state_out[(long)b * a.N + qs] = v;
      continue;
    }
    float y = 0.f;
    if (p < no) {
      // window sum of squares over the ABSOLUTE frames that cover the sample, in double, ascending
      const long sp = (long)e0 * a.hop + p, lo = sp - a.N + 1;
      const long t0 = lo > 0 ? (lo + a.hop - 1) / a.hop : 0;
      long t1 = sp / a.hop;
      if (t1 > (long)e0 + nf - 1) t1 = (long)e0 + nf - 1;
      if (t0 <= t1) {                            // a sample no frame covers stays +0
        double wss = 0.0;
        for (long t = t0; t <= t1; ++t) wss += a.win2[(int)(sp - t * a.hop)];
        const float acc = ola_sum(a, b, nf, p);
        const float w = (float)wss;
        y = w > IS_F32_TINY ? acc / w : acc;
        if (a.scale) y *= a.scale[b];
      }
    }
    a.out[(long)b * a.L + p] = y;
  }
}

bool is_desc_ok(const avvad_istft_stream_desc* d) {
  return d && d->B > 0 && d->T >= 0 && d->L >= 0 && frames::ok_n_fft(d->n_fft) && d->hop >= 1 &&
         d->hop <= d->n_fft && d->M >= 0 && d->mask_mode >= 0 && d->mask_mode <= 3 && (long)d->T * d->hop < (1L << 30) &&
         (long)d->B * d->T < (1L << 31) - 64 && (long)d->B * ((long)d->L + d->n_fft) < (1L << 40);
}
size_t is_lds_bytes(int K, int NG) {
  const size_t frames = (size_t)16 * NG * (K + IS_PAD) * sizeof(float), parts = (size_t)NG * IS_NW * 64 * sizeof(f32x4);
  return frames > parts ? frames : parts;      // both multiples of 16 bytes
}
size_t is_tab_bytes(int NG) { return align_up((size_t)(2 * 16 * NG + 1) * sizeof(int), 16); }
size_t is_basis_floats(int n_fft) { return (size_t)n_fft * n_fft; }

template <int NG, bool SIG>
int is_launch(const IsArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  if (int rc = allow_large_lds<is_product_kernel<NG, SIG>>(lds, IS_LDS_MAX)) return rc;
  hipLaunchKernelGGL((is_product_kernel<NG, SIG>), grid, dim3(IS_NT), lds, s, a);
  return AVVAD_OK;
}

}  // namespace

extern "C" size_t avvad_istft_stream_basis_bytes(int n_fft) {
  if (!frames::ok_n_fft(n_fft) || is_lds_bytes(n_fft, 1) + is_tab_bytes(1) > IS_LDS_MAX) return 0;
  return is_basis_floats(n_fft) * sizeof(float) + (size_t)n_fft * sizeof(double);
}

extern "C" int avvad_istft_stream_basis(int n_fft, float* out, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!out || !avvad_istft_stream_basis_bytes(n_fft) || ws_misaligned(out)) return AVVAD_EINVAL;
  const long n = (long)is_basis_floats(n_fft);
  hipLaunchKernelGGL(is_basis_kernel, dim3(frames::grid1(n)), dim3(256), 0, (hipStream_t)sv, out,
                     reinterpret_cast<double*>(out + n), n_fft, n);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

// workspace: Y [B T][n_fft]
extern "C" size_t avvad_istft_stream_workspace(const avvad_istft_stream_desc* d) {
  if (!is_desc_ok(d) || !avvad_istft_stream_basis_bytes(d->n_fft)) return 0;
  return align_up((size_t)d->B * (d->T > 0 ? d->T : 1) * d->n_fft, 64) * sizeof(float);
}

extern "C" int avvad_istft_stream(const float* spec, const float* mask, const int* n_frames, const int* n_before, const int* n_out,
                                  const float* scale, const float* state_in, float* state_out, const float* basis, float* out,
                                  const avvad_istft_stream_desc* d, void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!n_frames || !n_before || !n_out || !state_in || !state_out || !basis || !wsv || !is_desc_ok(d) ||
      !avvad_istft_stream_basis_bytes(d->n_fft) || state_in == state_out || (d->T > 0 && !spec) || (d->L > 0 && !out) ||
      (d->mask_mode != 0 && d->T > 0 && !mask) || ws_misaligned(wsv) || ws_misaligned(basis))
    return AVVAD_EINVAL;
  if (ws_bytes < avvad_istft_stream_workspace(d)) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  const int K = d->n_fft;
  float* Y = (float*)wsv;
  if (d->T > 0) {
    const long hint = d->M > 0 ? d->M : (long)d->B * d->T;
    int NG = hint > 16 ? 2 : 1;
    if (NG == 2 && is_lds_bytes(K, 2) + is_tab_bytes(2) > IS_LDS_MAX) NG = 1;
    long ny = (hint + 16 * NG - 1) / (16 * NG);
    ny = ny < 1 ? 1 : (ny > 16 ? 16 : ny);       // the passes beyond walk the grid's second dimension
    IsArgs a{spec, mask, n_frames, basis, Y, d->B, d->T, K, K / 2 + 1, d->mask_mode, (int)(is_lds_bytes(K, NG) / sizeof(float))};
    const dim3 grid(K / 16, (int)ny);
    const size_t lds = is_lds_bytes(K, NG) + is_tab_bytes(NG);
    const bool sig = d->mask_mode == 2;
    const int rc = NG == 2 ? (sig ? is_launch<2, true>(a, grid, lds, s) : is_launch<2, false>(a, grid, lds, s))
                           : (sig ? is_launch<1, true>(a, grid, lds, s) : is_launch<1, false>(a, grid, lds, s));
    if (rc) return rc;
  }
  OlaArgs o{Y, reinterpret_cast<const double*>(basis + is_basis_floats(K)), n_frames, n_before, n_out, scale, state_in, state_out,
            out, d->B, d->T, K, d->hop, d->L};
  hipLaunchKernelGGL(is_ola_kernel, dim3(frames::grid1((long)d->B * ((long)d->L + K))), dim3(256), 0, s, o);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
