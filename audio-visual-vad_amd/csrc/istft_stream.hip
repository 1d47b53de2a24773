// istft_stream.hip -- the masked inverse STFT on a stream of frames.  A call takes the next few frames of every row's
// spectrum (as avvad_stft_stream_fwd_spec hands them out) and a mask, and emits the samples that no later frame can cover
// any more; each row's unfinished overlap-add sums travel from call to call in a [B][n_fft] state.
//
// Two launches.  (1) The product Y[(b,t)][n] = sum_c A[(b,t)][c] Winv[c][n]: M = a handful of frames against K = N = n_fft,
// the basis-streaming product of stream_product.h with one plane.  Workgroup blockIdx.x owns 16 output-sample columns n;
// the pass's frames sit in LDS with the mask multiplied in while they are staged -- the masked spectrum never exists in
// memory.  (2) The overlap-add: one thread per output sample and per state element.  One frame's 16 columns overlap-add
// into other workgroups' columns unless hop divides n_fft, and a fusion in which a workgroup owned a residue class of
// samples would leave hop / 16 workgroups; hence the second launch.
//
// REAL-FFT PACKING.  The inverse of a half spectrum ignores im[0] and im[n_fft/2], so the contraction is packed to exactly
// K = n_fft rows: c = 0 is re[0], c = 1 is re[n_fft/2], c = 2f, 2f + 1 are re[f], im[f] for 1 <= f < n_fft/2.  K is then a
// multiple of 32, not n_fft + 2.
//
// SUMMATION ORDER.  Y[(b,t)][n] is summed as stream_product.h fixes it.  An output sample is the chain
// state + Y[b,0] + Y[b,1] + ... in ascending frame order; the state is that chain cut at the call boundary, and it starts
// at +0.  So the sum of one sample is the whole-utterance chain of overlap_add (istft.hip) for every split of a stream
// into calls: the same bits.
#include "stream_product.h"

namespace {

namespace sp = sprod;

constexpr int IS_E0_MAX = 1 << 30;  // frames a row may have behind it
constexpr int IS_SLOT_INTS = 2;     // per frame slot of a pass: row, frame of the row

struct IsArgs {
  const float *spec, *mask;
  const int* n_frames;
  const float* basis;
  float* Y;
  int B, T, K, F, mode;
  int tab;                  // float offset of the per-frame tables in LDS
};

// packed basis [column block][kk][lane][4]: element (c, n) of the windowed inverse real DFT, c the packed contraction row;
// behind it hann^2 as n_fft doubles
__global__ void is_basis_kernel(float* __restrict__ W, double* __restrict__ win2, int N, long n_el) {
  const int KQ = N >> 4;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n_el; idx += (long)gridDim.x * blockDim.x) {
    const int j = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    const long r = idx >> 8;
    const int kk = (int)(r % KQ), nb = (int)(r / KQ);
    const int c = sp::operand_index(N, kk, lane >> 4, j), n = 16 * nb + (lane & 15);
    const int f = c == 0 ? 0 : (c == 1 ? N / 2 : c >> 1);
    W[idx] = frames::idft_element(f, c >= 2 && (c & 1), n, N);
    if (idx < N) {
      const double w = frames::hann((int)idx, N);
      win2[idx] = w * w;
    }
  }
}

// SIG: frames::apply_mask's
template <int NG, bool SIG>
__global__ void __launch_bounds__(sp::NT) is_product_kernel(const IsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int FP = 16 * NG;
  const sp::Tables<FP, IS_SLOT_INTS> tb(lds + a.tab);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, P = K + sp::PAD, nb = blockIdx.x;
  const f32x4* wb = reinterpret_cast<const f32x4*>(a.basis) + ((long)nb * (K >> 4)) * 64 + lane;

  for (int pass = blockIdx.y;; pass += gridDim.y) {
    const int nfp = sp::map_frames(tb, a.B, pass * FP, [&](int b) { return clamp_count(a.n_frames[b], a.T); }, [](int) {});
    if (nfp <= 0) break;                         // uniform
    // ---- stage the frames in the packed order, times the mask (wave w takes frames w, w + 8, ...)
    for (int fr = wave; fr < nfp; fr += sp::NW) {
      float* dst = lds + fr * P;
      const long m = (long)tb.fb[fr] * a.T + tb.ft[fr];
      const float* src = a.spec + m * a.F * 2;
      const float* mk = a.mask + m * a.F;
#pragma unroll 4
      for (int c = lane; c < K; c += 64) {
        const int f = c == 0 ? 0 : (c == 1 ? K >> 1 : c >> 1);
        float v = src[c == 1 ? K : c];           // (re, im) adjacent: re[f] at 2f, im[f] at 2f + 1
        if (a.mode) v = frames::apply_mask<SIG>(v, mk[f], a.mode);
        dst[c] = v;
      }
    }
    __syncthreads();
    sp::product<NG, 1>(lds, wb, K, nfp);
    // ---- thread (frame, column) finishes one value: the 16 columns of a frame are one 64-byte store
    const int fr = tid >> 4, col = tid & 15;
    if (fr < nfp) {                              // column col is register col & 3 of lane quarter col >> 2
      const float y = sp::finish<1>(lds, fr >> 4, 0, (fr & 15) + 16 * (col >> 2), col & 3);
      a.Y[((long)tb.fb[fr] * a.T + tb.ft[fr]) * K + 16 * nb + col] = y;
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
  const frames::Cover c = frames::covering(p, a.N, a.hop, nf - 1);
  for (int i = (int)c.t0; i <= (int)c.t1; ++i) acc += a.Y[((long)b * a.T + i) * a.N + (int)(p - (long)i * a.hop)];
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
    const int nf = clamp_count(a.n_frames[b], a.T), e0 = clamp_count(a.n_before[b], IS_E0_MAX), no = clamp_count(a.n_out[b], a.L);
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
      const long s = (long)e0 * a.hop + p;
      const frames::Cover c = frames::covering(s, a.N, a.hop, (long)e0 + nf - 1);
      if (c.t0 <= c.t1) {                        // a sample no frame covers stays +0
        double wss = 0.0;
        for (long t = c.t0; t <= c.t1; ++t) wss += a.win2[(int)(s - t * a.hop)];
        y = frames::ola_normalise(ola_sum(a, b, nf, p), wss);
        if (a.scale) y *= a.scale[b];
      }
    }
    a.out[(long)b * a.L + p] = y;
  }
}

bool is_desc_ok(const avvad_istft_stream_desc* d) {
  return d && d->B > 0 && d->T >= 0 && d->L >= 0 && frames::ok_n_fft(d->n_fft) && d->n_fft <= sp::K_MAX && d->hop >= 1 &&
         d->hop <= d->n_fft && d->M >= 0 && d->mask_mode >= 0 && d->mask_mode <= 3 && (long)d->T * d->hop < (1L << 30) &&
         (long)d->B * d->T < (1L << 31) - 64 && (long)d->B * ((long)d->L + d->n_fft) < (1L << 40);
}
// the product's plan for about `hint` frames: one plane
sp::Plan is_plan(int n_fft, long hint) { return sp::plan(n_fft, 1, IS_SLOT_INTS, hint); }
size_t is_basis_floats(int n_fft) { return (size_t)n_fft * n_fft; }

}  // namespace

extern "C" size_t avvad_istft_stream_basis_bytes(int n_fft) {
  if (!frames::ok_n_fft(n_fft) || n_fft > sp::K_MAX || !is_plan(n_fft, 1).NG) return 0;
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
    const sp::Plan p = is_plan(K, d->M > 0 ? d->M : (long)d->B * d->T);
    IsArgs a{spec, mask, n_frames, basis, Y, d->B, d->T, K, K / 2 + 1, d->mask_mode, p.tab};
    const dim3 grid(K / 16, p.ny);
    const bool sig = d->mask_mode == 2;
    const int rc = p.NG == 2 ? (sig ? sp::launch<is_product_kernel<2, true>>(a, grid, p.lds, s)
                                    : sp::launch<is_product_kernel<2, false>>(a, grid, p.lds, s))
                             : (sig ? sp::launch<is_product_kernel<1, true>>(a, grid, p.lds, s)
                                    : sp::launch<is_product_kernel<1, false>>(a, grid, p.lds, s));
    if (rc) return rc;
  }
  OlaArgs o{Y, reinterpret_cast<const double*>(basis + is_basis_floats(K)), n_frames, n_before, n_out, scale, state_in, state_out,
            out, d->B, d->T, K, d->hop, d->L};
  hipLaunchKernelGGL(is_ola_kernel, dim3(frames::grid1((long)d->B * ((long)d->L + K))), dim3(256), 0, s, o);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
