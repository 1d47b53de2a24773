// lip.hip -- the video front-end: NTCD-TIMIT lip-region DCT coefficients -> the 67x67 crops the trunk consumes, at the
// STFT's frame rate, on the GPU.
//
// Replaces the offline producer of the reference, scripts/create_video_train_files_upsampled.py:105-173
// (process_write_video: scipy idct twice per frame, min / max-range normalisation over the utterance, np.rot90(., 3), an
// ffmpeg `fps` filter through a temporary mp4) and its pixel statistics (:294-310, :350-361).
//
// Per utterance b with N_b coefficient rows X_n (67x67, row-major):
//   A_n   = C X_n C^T,           C[k][m] = 1 (m == 0), 2 cos(pi (2k+1) m / 134)      (scipy's unnormalised type-2 idct)
//   V_n   = (A_n - gmin) / R * 255,   gmin = min over the utterance, R = max_n (max A_n - min A_n);  R == 0: V = 0
//   out_n = rot90(V_n, 3):  out[i][j] = V[66 - j][i], i.e. out = C X^T C'^T with C' = C with its rows reversed
//   quantise (optional): clip to [0, 255], round towards zero
//   output frame k shows input frame i for s(i) <= k < s(i+1), s(i) = (2 i p + q) / (2 q), cut at min(s(N_b), n_out[b])
//
// Kernels:
//   dct_table   Ct[a][i] = C[i][a] (pitch 68, zero padded) from double cosines, into the workspace.
//   lip_frames  one wave per coefficient frame, four frames per workgroup, a persistent grid of one workgroup per CU: the
//               frame is staged into the wave's LDS buffer with 16-byte loads (the next frame's are in flight during the
//               products); Z = X^T C'^T and out = C Z are two fp32 MFMA products (v_mfma_f32_16x16x4_f32, 67 padded to 80:
//               25 accumulator tiles; both fp32 MFMA shapes run at 64 FLOP per clock and SIMD, so the 80-pad does 1.44x
//               less work than the 96-pad of 32x32x2); Z goes through the same LDS buffer.  The frame's min / max and the
//               unnormalised rotated frame A (through LDS, whole-line stores) go to the workspace.
//   lip_utt     per utterance: gmin, 255 / R, the output length.  min / max in any order are the same bits.
//   lip_write   one workgroup per input frame: A -> normalise, quantise, the frame's (sum, sumsq) in double times its number
//               of output slots -> one partial per input frame, and the frame stored to each of its s(i+1) - s(i) slots
//               (standardised on the way when mean / std are given).  Memory-bound: 18 KB in, 37 KB out per input frame.
//   lip_pad     zeroes the frames k >= length of the padded batch.
//   lip_add     adds the partials to the accumulator in a fixed order (a function of the shape alone) + the pixel count.
// The normalisation needs gmin and R before a frame can be written.  Both forms were built and measured (B = 64, 9540 input
// frames): running the two products twice (a min / max pass, then a writing pass) took 0.52 ms, materialising A and
// re-reading it 0.365 ms -- the products, not the bytes, bound lip_frames, so the 2 x 18 KB per frame are the cheaper price.
// No floating-point atomics; the partials are per input frame, so results do not depend on the grid ("max_cus").
#include <math.h>

#include "reduce.h"

namespace {

constexpr int W = 67, NPIX = W * W;      // 4489 values per frame
constexpr int LD = 68;                   // pitch of the table and of the intermediate: K = 67 padded to 17 steps of 4
constexpr int BUF = LD * LD;             // floats of the table / of one wave's buffer (18.1 KB)
constexpr int NT = 5, KS = LD / 4;       // 5 x 5 tiles of 16 x 16, 17 k-steps
constexpr int RAWQ = 18;                 // float4 per lane that cover a frame from the 16-byte boundary below it (<= 1123)

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// LDS traffic inside one wave: the hardware executes a wave's LDS instructions in order; this keeps the compiler from
// moving a read of another lane's value above the write
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// frames of utterance b that lie inside coef [rows][NPIX], whatever the device arrays say
__device__ __forceinline__ int valid_frames(int st, int n, long rows) {
  if (st < 0 || n <= 0 || st >= rows) return 0;
  return (int)min((long)n, rows - st);
}
__device__ __forceinline__ long frame_start(long i, int p, int q) { return (2 * i * p + q) / (2 * (long)q); }

__global__ void dct_table(float* __restrict__ Ct) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= BUF) return;
  const int a = idx / LD, i = idx - a * LD;
  float v = 0.f;
  if (a < W && i < W) v = a == 0 ? 1.f : (float)(2.0 * cospi((double)(((2 * i + 1) * a) % (4 * W)) / (double)(2 * W)));
  Ct[idx] = v;
}

// the float4s of frame `row` counted from the 16-byte boundary at or below its first value; nothing outside the frame or
// the tensor is read
__device__ __forceinline__ void load_raw(float4 (&raw)[RAWQ], const float* __restrict__ coef, long row, int lane) {
  const int s = (int)(row & 3);          // NPIX % 4 == 1
  const float* base = coef + (row * NPIX - s);
#pragma unroll
  for (int u = 0; u < RAWQ; ++u) {
    const int e = 4 * (u * 64 + lane) - s;                       // first value of this float4, relative to the frame
    if (e >= 0 && e + 3 < NPIX) raw[u] = *reinterpret_cast<const float4*>(base + e + s);
    else {
      float t[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = (e + c >= 0 && e + c < NPIX) ? base[e + s + c] : 0.f;
      raw[u] = make_float4(t[0], t[1], t[2], t[3]);
    }
  }
}

__global__ void __launch_bounds__(256)
    lip_frames(const float* __restrict__ coef, long rows, const int* __restrict__ starts, const int* __restrict__ n_in,
               const float* __restrict__ Ctg, float* __restrict__ flo, float* __restrict__ fhi, float* __restrict__ Aout) {
  __shared__ __attribute__((aligned(16))) float tab[BUF];
  __shared__ __attribute__((aligned(16))) float bufs[4][BUF];
  for (int idx = threadIdx.x; idx < BUF; idx += 256) tab[idx] = Ctg[idx];
  __syncthreads();                       // the only workgroup barrier: every wave is here
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* xb = bufs[wv];
  const int b = blockIdx.y;
  const int st = starts[b], n = valid_frames(st, n_in[b], rows);
  const int stride = gridDim.x * 4;
  int i = blockIdx.x * 4 + wv;
  if (i >= n) return;
  const int l15 = lane & 15, l4 = lane >> 4;
  float4 raw[RAWQ];
  load_raw(raw, coef, (long)st + i, lane);
  for (; i < n; i += stride) {
    const long row = (long)st + i;
    const int s = (int)(row & 3);
#pragma unroll
    for (int u = 0; u < RAWQ; ++u) reinterpret_cast<float4*>(xb)[u * 64 + lane] = raw[u];     // 18 * 64 * 4 = 4608 <= BUF
    if (i + stride < n) load_raw(raw, coef, row + stride, lane);
    wave_sync();
    f32x4 acc[NT][NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
      for (int tj = 0; tj < NT; ++tj) acc[ti][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
    // Z[bb][j] = sum_a X[a][bb] C[66 - j][a]:  A operand X^T (lane: row bb, k = a), B operand the reversed table
#pragma unroll 2
    for (int ks = 0; ks < KS; ++ks) {
      const int k = 4 * ks + l4;
      float av[NT], bv[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = t * 16 + l15;
        const bool on = c < W;
        av[t] = (on && k < W) ? xb[on && k < W ? s + k * W + c : 0] : 0.f;
        bv[t] = on ? tab[on ? k * LD + (W - 1 - c) : 0] : 0.f;                                 // row 67 of the table is zero
      }
#pragma unroll
      for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) acc[ti][tj] = mfma16(av[ti], bv[tj], acc[ti][tj]);
    }
    wave_sync();                         // X is read; Z takes its place (rows / columns 67 are exact zeros)
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
      for (int tj = 0; tj < NT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rr = ti * 16 + 4 * l4 + r, cc = tj * 16 + l15;
          if (rr < LD && cc < LD) xb[rr * LD + cc] = acc[ti][tj][r];
          acc[ti][tj][r] = 0.f;
        }
    wave_sync();
    // out[ii][j] = sum_bb C[ii][bb] Z[bb][j]
#pragma unroll 2
    for (int ks = 0; ks < KS; ++ks) {
      const int k = 4 * ks + l4;
      float av[NT], bv[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = t * 16 + l15;
        const bool on = c < W;
        av[t] = on ? tab[on ? k * LD + c : 0] : 0.f;
        bv[t] = on ? xb[on ? k * LD + c : 0] : 0.f;
      }
#pragma unroll
      for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) acc[ti][tj] = mfma16(av[ti], bv[tj], acc[ti][tj]);
    }
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
      for (int tj = 0; tj < NT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ti * 16 + 4 * l4 + r < W && tj * 16 + l15 < W) mn = fminf(mn, acc[ti][tj][r]), mx = fmaxf(mx, acc[ti][tj][r]);
    mn = wave_fold(mn, fminf), mx = wave_fold(mx, fmaxf);
    if (lane == 0) flo[row] = mn, fhi[row] = mx;
    wave_sync();                         // Z is read; the frame takes its place, row-major with pitch 67, for whole-line stores
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
      for (int tj = 0; tj < NT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rr = ti * 16 + 4 * l4 + r, cc = tj * 16 + l15;
          if (rr < W && cc < W) xb[rr * W + cc] = acc[ti][tj][r];
        }
    wave_sync();
    float* dst = Aout + row * NPIX;
    for (int e = lane; e < NPIX; e += 64) dst[e] = xb[e];
    wave_sync();
  }
}

__global__ void __launch_bounds__(256)
    lip_utt(const float* __restrict__ flo, const float* __restrict__ fhi, const int* __restrict__ starts, const int* __restrict__ n_in,
            const int* __restrict__ n_out, long rows, int T, int p, int q, float* __restrict__ gmin, float* __restrict__ inv,
            int* __restrict__ out_len) {
  __shared__ float smn[4];
  __shared__ double srg[4];
  const int b = blockIdx.x, st = starts[b], n = valid_frames(st, n_in[b], rows);
  float mn = INFINITY;
  double rg = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float lo = flo[(long)st + i], hi = fhi[(long)st + i];
    mn = fminf(mn, lo);
    rg = fmax(rg, (double)hi - (double)lo);
  }
  const auto most = [](double a, double b) { return fmax(a, b); };
  fold4_put(smn, mn, fminf);
  fold4_put(srg, rg, most);
  __syncthreads();
  if (threadIdx.x == 0) {
    mn = fold4_get(smn, fminf);
    rg = fold4_get(srg, most);
    gmin[b] = n > 0 ? mn : 0.f;
    inv[b] = rg > 0.0 ? (float)(255.0 / rg) : 0.f;               // R == 0 (constant frames): the frames are written as 0
    long len = frame_start(n, p, q);
    if (n_out) len = min(len, (long)max(n_out[b], 0));
    out_len[b] = (int)min(len, (long)T);
  }
}

// One workgroup per input frame: the materialised frame A -> normalise, quantise, partial statistics, its output slots.
__global__ void __launch_bounds__(256)
    lip_write(const float* __restrict__ A, long rows, const int* __restrict__ starts, const int* __restrict__ n_in,
              const float* __restrict__ gmin, const float* __restrict__ inv, const int* __restrict__ out_len, float* __restrict__ video,
              double* __restrict__ part, int T, int p, int q, int quantize, const float* __restrict__ mean, const float* __restrict__ stdv,
              float eps) {
  __shared__ double red[2][4];
  const int b = blockIdx.y, i = blockIdx.x;
  const int st = starts[b], n = valid_frames(st, n_in[b], rows);
  if (i >= n) return;
  const long row = (long)st + i;
  const int lim = min(out_len[b], T);
  const int k0 = (int)min(frame_start(i, p, q), (long)lim), k1 = (int)min(frame_start((long)i + 1, p, q), (long)lim);
  if (k1 <= k0) {                        // a frame the length cap cuts off: nothing to write, nothing to count
    if (part && threadIdx.x == 0) part[2 * row] = 0.0, part[2 * row + 1] = 0.0;
    return;
  }
  const float g = gmin[b], sc = inv[b];
  float mu = 0.f, den = 1.f;
  if (mean) mu = mean[0], den = stdv[0] + eps;
  const float* src = A + row * NPIX;
  float* dst = video + ((long)b * T + k0) * NPIX;
  double s1 = 0.0, s2 = 0.0;
  for (int e = threadIdx.x; e < NPIX; e += 256) {
    float v = __fmul_rn(__fsub_rn(src[e], g), sc);
    if (quantize) v = truncf(fminf(fmaxf(v, 0.f), 255.f));
    s1 += (double)v;
    s2 += (double)v * (double)v;
    if (mean) v = (v - mu) / den;
    for (int k = 0; k < k1 - k0; ++k) dst[(long)k * NPIX + e] = v;
  }
  if (!part) return;                     // statistics of what is stored, before the standardisation
  const double s[2] = {s1, s2};
  fold4_put(red, s, Add());
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * row] = (double)(k1 - k0) * fold4_get(red[0], Add());
    part[2 * row + 1] = (double)(k1 - k0) * fold4_get(red[1], Add());
  }
}

__global__ void __launch_bounds__(256) lip_pad(const int* __restrict__ out_len, float* __restrict__ video, int T) {
  const int k = blockIdx.x, b = blockIdx.y;
  if (k < out_len[b]) return;
  float* dst = video + ((long)b * T + k) * NPIX;
  for (int e = threadIdx.x; e < NPIX; e += 256) dst[e] = 0.f;
}

// acc += (sum, sumsq) of the frames' partials, count += written pixels.  Wave w takes the utterances w, w + 16, ..., lane l
// their frames l, l + 64, ... in ascending order; the lanes are added by butterflies (reduce.h) and the sixteen waves in
// ascending order.  (One utterance after the other over the whole workgroup is a chain of B dependent load rounds: 34 us for B = 64.)
__global__ void __launch_bounds__(1024)
    lip_add(const double* __restrict__ part, const int* __restrict__ starts, const int* __restrict__ n_in, const int* __restrict__ out_len,
            long rows, int B, double* __restrict__ acc) {
  __shared__ double red[2][16];
  __shared__ long long cnt[16];
  double s1 = 0.0, s2 = 0.0;
  long long c = 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int b = wv; b < B; b += 16) {
    const int st = starts[b], n = valid_frames(st, n_in[b], rows);
    const double2* pp = reinterpret_cast<const double2*>(part) + st;
    for (int i = lane; i < n; i += 64) {
      const double2 v = pp[i];
      s1 += v.x, s2 += v.y;
    }
  }
  for (int b = threadIdx.x; b < B; b += 1024) c += (long long)out_len[b] * NPIX;
  s1 = wave_sum(s1), s2 = wave_sum(s2), c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = s1, red[1][threadIdx.x >> 6] = s2, cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a1 = 0.0, a2 = 0.0;
    long long tot = 0;
    for (int w = 0; w < 16; ++w) a1 += red[0][w], a2 += red[1][w], tot += cnt[w];
    acc[0] += a1, acc[1] += a2, acc[2] += (double)tot;
  }
}

inline bool ok_desc(const avvad_lip_desc* d) {
  return d && d->B > 0 && d->B <= 65535 && d->rows > 0 && d->rows < (1L << 31) && d->n_max > 0 && d->T > 0 && d->T <= 65535 &&
         d->W == W && d->H == W && d->p > 0 && d->q > 0 && d->p < (1 << 20) && d->q < (1 << 20);
}
struct Carve { size_t tab, flo, fhi, gmin, inv, part, A, total; };
inline Carve carve(const avvad_lip_desc* d) {
  Carve c;
  size_t o = 0;
  c.tab = o, o += align_up(BUF * sizeof(float), 256);
  c.flo = o, o += align_up((size_t)d->rows * sizeof(float), 256);
  c.fhi = o, o += align_up((size_t)d->rows * sizeof(float), 256);
  c.gmin = o, o += align_up((size_t)d->B * sizeof(float), 256);
  c.inv = o, o += align_up((size_t)d->B * sizeof(float), 256);
  c.part = o, o += align_up((size_t)d->rows * 2 * sizeof(double), 256);
  c.A = o, o += align_up((size_t)d->rows * NPIX * sizeof(float), 256);
  c.total = o;
  return c;
}

}  // namespace

extern "C" size_t avvad_lip_decode_workspace(const avvad_lip_desc* d) { return ok_desc(d) ? carve(d).total : 0; }

extern "C" int avvad_lip_decode(const float* coef, const int* starts, const int* n_in, const int* n_out, float* video, int* out_len,
                                double* acc, const float* mean, const float* std_, const avvad_lip_desc* d, void* wsv, size_t ws_bytes,
                                avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!coef || !starts || !n_in || !video || !out_len || !wsv || !ok_desc(d)) return AVVAD_EINVAL;
  if (((uintptr_t)coef & 15) || ((uintptr_t)wsv & 15) || ((uintptr_t)acc & 7) || (mean == nullptr) != (std_ == nullptr)) return AVVAD_EINVAL;
  const Carve c = carve(d);
  if (ws_bytes < c.total) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  char* ws = (char*)wsv;
  float *tab = (float*)(ws + c.tab), *flo = (float*)(ws + c.flo), *fhi = (float*)(ws + c.fhi), *gmin = (float*)(ws + c.gmin),
        *inv = (float*)(ws + c.inv);
  double* part = acc ? (double*)(ws + c.part) : nullptr;
  const int cus = avvad_tune().max_cus > 0 ? avvad_tune().max_cus : 256;      // (not grid_cus(): no upper clamp here, kept as behaviour)
  const int gx = max(1, min(cdiv(d->n_max, 4), cus / d->B));      // one resident workgroup per CU; a wave walks its frames
  hipLaunchKernelGGL(dct_table, dim3(cdiv(BUF, 256)), dim3(256), 0, s, tab);
  float* A = (float*)(ws + c.A);
  hipLaunchKernelGGL(lip_frames, dim3(gx, d->B), dim3(256), 0, s, coef, d->rows, starts, n_in, tab, flo, fhi, A);
  hipLaunchKernelGGL(lip_utt, dim3(d->B), dim3(256), 0, s, flo, fhi, starts, n_in, n_out, d->rows, d->T, d->p, d->q, gmin, inv, out_len);
  hipLaunchKernelGGL(lip_write, dim3(d->n_max, d->B), dim3(256), 0, s, A, d->rows, starts, n_in, gmin, inv, out_len, video, part, d->T,
                     d->p, d->q, d->quantize, mean, std_, d->norm_eps);
  hipLaunchKernelGGL(lip_pad, dim3(d->T, d->B), dim3(256), 0, s, out_len, video, d->T);
  if (acc) hipLaunchKernelGGL(lip_add, dim3(1), dim3(1024), 0, s, part, starts, n_in, out_len, d->rows, d->B, acc);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
