// stats.hip -- train-set standardisation statistics on the GPU: per-bin (or one scalar) sum / sum of squares / count of
// the network inputs, accumulated over a whole training set batch by batch, and mean / empirical std from them.
//
// Replaces the offline producers of the reference:
//   scripts/create_audio_train_files.py:196-214, 273-280, 340-392   (n_samples, channels_sum, channels_squared_sum per file,
//                                                                    mean = sum / n, std = sqrt((sumsq - n mean^2) / (n - 1)))
//   scripts/create_video_train_files_upsampled.py                   (the same triple over all pixels of all frames)
// which write the statistics into HDF5.  The reference keeps sum and sumsq in float32 (an accident of `0. + float32
// array`); here everything behind the float32 feature value is double.
//
// An accumulator is 2 * nstat + 1 doubles in caller-owned device memory: sum[nstat], sumsq[nstat], count.  Calls ADD to it.
//
// Kernel forms (memory-bound: one read of the data, nothing else of that size):
//   column_partials<Load>: rows are cut into chunks of ROWS_PER_CHUNK; workgroup (chunk, column block) has four
//        waves, each walks a quarter of the chunk's rows with its 64 lanes along the bin axis (a wave reads 1024 / 256
//        consecutive bytes per row, eight rows in flight), widens every value to double and keeps (sum, sumsq) per bin;
//        the four waves are added through LDS in wave order and the workgroup stores its partial pairs.  Load = SpectrumLogPower reads the DFT
//        GEMM's S [rows][ld] as (re, im) pairs and forms log(re^2 + im^2 + eps) as stft.hip's power_log does -- the
//        [B][T][F] feature tensor is never written; Load = PlainFeature reads materialised features x [rows][F].
//   scalar_partials: nstat == 1 (video): a chunk of rows is one workgroup; lanes stride over a row's F values, cross-lane
//        and cross-wave sums in a fixed order (reduce.h).
//   add_partials: adds the chunks' partials into the accumulator in a fixed order (sixteen contiguous segments of chunks,
//        each ascending, then the segments ascending); one extra workgroup counts the valid rows (integers).
// No floating-point atomics, and the chunking depends on the shape alone: results are bit-identical run to run and
// whatever the CU cap.  Rows t >= lengths[b] (which hold log(eps) after the DFT of zero padding) are skipped.
#include <math.h>

#include "frames.h"
#include "reduce.h"

namespace {

constexpr int ROWS_PER_CHUNK = 128;      // rows of one partial (per-column form): 32 per wave
constexpr int SCALAR_CHUNK_ELEMS = 16384;  // nstat == 1: values of one partial, rounded down to whole rows (at least one)

// S [rows][ld] of (re, im) pairs -> log(re^2 + im^2 + eps): power_log's expression (stft.hip), rounded after every
// operation.  That is the code hipcc emits for power_log wherever a thread handles one element (batches up to 2^20
// values, its grid-stride loop's remainder form), so the statistics are those of the features avvad_stft returns, bit
// for bit; in the 2x-unrolled body of larger batches hipcc contracts re*re + im*im to fma(re, re, im*im) for the elements
// it pairs, a last-bit difference in their power that the features themselves carry from element to element.
struct SpectrumLogPower {                // a lane takes two neighbouring bins: one 16-byte load
  static constexpr int NB = 2;
  typedef float4 Raw;
  const float* S;
  int ld;
  float eps;
  __device__ __forceinline__ Raw fetch(long m, int f) const { return *reinterpret_cast<const float4*>(S + m * ld + 2 * f); }
  __device__ __forceinline__ float value(Raw c, int i) const {
    const float re = i ? c.z : c.x, im = i ? c.w : c.y;
    const float pw = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
    return logf(__fadd_rn(pw, eps));
  }
};
struct PlainFeature {                    // x [rows][F]: rows of an odd F are not 16-byte aligned, one value per lane
  static constexpr int NB = 1;
  typedef float Raw;
  const float* x;
  int F;
  __device__ __forceinline__ Raw fetch(long m, int f) const { return x[m * F + f]; }
  __device__ __forceinline__ float value(Raw v, int) const { return v; }
};

__device__ __forceinline__ bool row_counts(const int* __restrict__ lengths, int T, long m) {
  if (!lengths) return true;
  const int b = (int)m / T;              // rows < 2^31 (launch precondition)
  return (int)m - b * T < lengths[b];
}

// part[chunk][2 * F]: sum at [f], sumsq at [F + f].  Workgroup (chunk, column block of 64 * NB bins); the spectrum's row
// pitch is a whole number of float4, so the second bin of the last lane may be a zero pad column: summed, never stored.
template <class Load>
__global__ void __launch_bounds__(256)
    column_partials(Load ld, long M, int T, int F, const int* __restrict__ lengths, double* __restrict__ part) {
  constexpr int NB = Load::NB, UN = 8;   // UN rows in flight per wave
  __shared__ double red[2][4][64 * NB];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // rows and their validity live in scalar registers
  const int f0 = (blockIdx.y * 64 + lane) * NB;
  const long m0 = (long)blockIdx.x * ROWS_PER_CHUNK + wv * (ROWS_PER_CHUNK / 4);
  const long m1 = min(M, m0 + ROWS_PER_CHUNK / 4);
  double s[NB] = {}, q[NB] = {};
  if (f0 < F) {
    // (utterance, frame) of the wave's rows advance with them: one division and one length load per utterance touched
    const bool ragged = lengths != nullptr;
    int b = ragged ? (int)m0 / T : 0, t = ragged ? (int)m0 - b * T : 0;
    int len = (ragged && m0 < m1) ? lengths[b] : 0;
    for (long m = m0; m < m1; m += UN) {
      typename Load::Raw raw[UN] = {};
      bool on[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        on[u] = m + u < m1 && (!ragged || t < len);
        if (ragged && ++t == T) {
          t = 0, ++b;
          if (m + u + 1 < m1) len = lengths[b];                        // the next row exists, so b < B
        }
      }
#pragma unroll
      for (int u = 0; u < UN; ++u)
        if (on[u]) raw[u] = ld.fetch(m + u, f0);
#pragma unroll
      for (int u = 0; u < UN; ++u)
        if (on[u]) {
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            const double x = (double)ld.value(raw[u], i);
            s[i] += x;
            q[i] += x * x;
          }
        }
    }
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) red[0][wv][lane * NB + i] = s[i], red[1][wv][lane * NB + i] = q[i];
  __syncthreads();
  if (wv == 0) {
    double* p = part + (long)blockIdx.x * 2 * F;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int f = f0 + i, j = lane * NB + i;
      if (f < F) {
        p[f] = ((red[0][0][j] + red[0][1][j]) + red[0][2][j]) + red[0][3][j];
        p[F + f] = ((red[1][0][j] + red[1][1][j]) + red[1][2][j]) + red[1][3][j];
      }
    }
  }
}

// part[chunk][2]: sum and sumsq over every value of the chunk's counted rows
__global__ void __launch_bounds__(256)
    scalar_partials(const float* __restrict__ x, long M, int T, int F, int rows_per_chunk, const int* __restrict__ lengths,
                    double* __restrict__ part) {
  __shared__ double red[2][4];
  const long m0 = (long)blockIdx.x * rows_per_chunk, m1 = min(M, m0 + rows_per_chunk);
  double s = 0.0, q = 0.0;
  for (long m = m0; m < m1; ++m) {
    if (!row_counts(lengths, T, m)) continue;
    const float* row = x + m * F;
    for (int f = threadIdx.x; f < F; f += 256) {
      const double v = (double)row[f];
      s += v;
      q += v * v;
    }
  }
  const double sq[2] = {s, q};
  fold4_put(red, sq, Add());
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * (long)blockIdx.x] = fold4_get(red[0], Add());
    part[2 * (long)blockIdx.x + 1] = fold4_get(red[1], Add());
  }
}

// acc[c] += the chunks' partials, c < 2 * nstat, in a fixed two-level order: the chunks are cut into ADD_WAVES contiguous
// segments (a function of the chunk count alone), wave w of the workgroup adds segment w in ascending chunk order with its
// 64 lanes along c (512 consecutive bytes per load, ADD_UNROLL loads in flight), and the segment sums are added to the
// accumulator in ascending segment order.  (One thread per statistic walking all chunks is a chain of dependent loads:
// measured 100 us for 370 chunks, twice the pass over the data.)  The last workgroup counts the valid rows instead.
constexpr int ADD_WAVES = 16, ADD_UNROLL = 8;
__global__ void __launch_bounds__(64 * ADD_WAVES)
    add_partials(const double* __restrict__ part, int nchunks, int nstat, const int* __restrict__ lengths, int B, int T,
                 double per_row, double* __restrict__ acc) {
  const int ncol = 2 * nstat;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (blockIdx.x + 1 < gridDim.x) {
    __shared__ double seg[ADD_WAVES][64];
    const int c = blockIdx.x * 64 + lane;
    const int per = (nchunks + ADD_WAVES - 1) / ADD_WAVES;
    const int k0 = wv * per, k1 = min(nchunks, k0 + per);
    double v = 0.0;
    if (c < ncol) v = add_ascending<ADD_UNROLL>(0.0, part + c, ncol, k0, k1);
    seg[wv][lane] = v;
    __syncthreads();
    if (wv == 0 && c < ncol) {
      double a = acc[c];
#pragma unroll
      for (int w = 0; w < ADD_WAVES; ++w) a += seg[w][lane];
      acc[c] = a;
    }
    return;
  }
  __shared__ long long red[ADD_WAVES];
  long long n = 0;                       // integers: exact in any order
  if (lengths)
    for (int b = threadIdx.x; b < B; b += 64 * ADD_WAVES) n += min(max(lengths[b], 0), T);
  else if (threadIdx.x == 0) n = (long long)B * T;
  n = wave_sum(n);
  if (lane == 0) red[wv] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long tot = 0;
    for (int w = 0; w < ADD_WAVES; ++w) tot += red[w];
    acc[ncol] += (double)tot * per_row;
  }
}

// mean = sum / n, std = sqrt(max((sumsq - n mean^2) / (n - 1), 0)) in double, stored as float; n < 2: NaN std
__global__ void finalize(const double* __restrict__ acc, int nstat, float* __restrict__ mean, float* __restrict__ stdv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nstat) return;
  const double n = acc[2 * nstat];
  const double mu = acc[i] / n;
  double var = (acc[nstat + i] - n * (mu * mu)) / (n - 1.0);
  if (var < 0.0) var = 0.0;              // constant data: the difference may round to a tiny negative number
  mean[i] = (float)mu;
  stdv[i] = n < 2.0 ? __builtin_nanf("") : (float)sqrt(var);
}

inline int scalar_rows_per_chunk(int F) { return F >= SCALAR_CHUNK_ELEMS ? 1 : SCALAR_CHUNK_ELEMS / F; }
inline long n_chunks(long rows, int F, int nstat) {
  const long per = (nstat == 1 && F != 1) ? scalar_rows_per_chunk(F) : ROWS_PER_CHUNK;
  return (rows + per - 1) / per;
}
inline bool ok_shape(long rows, int F, int nstat) {
  return rows > 0 && rows < (1L << 31) && F > 0 && (nstat == F || nstat == 1) && (F + 63) / 64 <= 65535 &&
         n_chunks(rows, F, nstat) < (1L << 31) / 2;
}
inline size_t partial_bytes(long rows, int F, int nstat) {
  return align_up((size_t)n_chunks(rows, F, nstat) * 2 * nstat * sizeof(double), 256);
}

template <class Load>
void launch_columns(Load ld, long rows, int T, int F, const int* lengths, double* part, hipStream_t s) {
  hipLaunchKernelGGL(column_partials<Load>, dim3((unsigned)n_chunks(rows, F, F), (F + 64 * Load::NB - 1) / (64 * Load::NB)),
                     dim3(256), 0, s, ld, rows, T, F, lengths, part);
}
void launch_add(const double* part, long rows, int F, int nstat, const int* lengths, int B, int T, double* acc, hipStream_t s) {
  hipLaunchKernelGGL(add_partials, dim3((2 * nstat + 63) / 64 + 1), dim3(64 * ADD_WAVES), 0, s, part, (int)n_chunks(rows, F, nstat), nstat,
                     lengths, B, T, nstat == F ? 1.0 : (double)F, acc);
}

}  // namespace

extern "C" size_t avvad_stats_workspace(size_t rows, int nstat) {
  // the per-column form's need; the scalar form (nstat == 1) never has more chunks than rows
  if (rows == 0 || rows >= ((size_t)1 << 31) || nstat <= 0) return 0;
  const size_t chunks = nstat == 1 ? rows : (rows + ROWS_PER_CHUNK - 1) / ROWS_PER_CHUNK;
  return align_up(chunks * 2 * (size_t)nstat * sizeof(double), 256);
}

extern "C" int avvad_stats_accumulate(const float* x, const int* lengths, double* acc, int B, int T, int F, int nstat, void* ws,
                                      size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!x || !acc || !ws || B <= 0 || T <= 0 || ws_misaligned(ws) || ((uintptr_t)acc & 7)) return AVVAD_EINVAL;
  const long rows = (long)B * T;
  if (!ok_shape(rows, F, nstat)) return AVVAD_EINVAL;
  if (ws_bytes < partial_bytes(rows, F, nstat)) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  double* part = (double*)ws;
  if (nstat == F) launch_columns(PlainFeature{x, F}, rows, T, F, lengths, part, s);
  else
    hipLaunchKernelGGL(scalar_partials, dim3((unsigned)n_chunks(rows, F, 1)), dim3(256), 0, s, x, rows, T, F, scalar_rows_per_chunk(F),
                       lengths, part);
  launch_add(part, rows, F, nstat, lengths, B, T, acc, s);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

// workspace of the fused call: the STFT's (basis, spectrum, GEMM slab: the spectrum is live while the partials are
// written) followed by the partials
static size_t partials_offset(const frames::SpecWs& w) { return align_up(w.total * sizeof(float), 256); }

extern "C" size_t avvad_stft_stats_workspace(const avvad_stft_desc* d) {
  if (!frames::ok_desc(d)) return 0;
  const long rows = (long)d->B * d->T;
  const int F = d->n_fft / 2 + 1;
  const frames::SpecWs w = frames::spec_ws(d->n_fft, rows);
  if (!ok_shape(rows, F, F) || rows * w.ld >= (1L << 31)) return 0;
  return partials_offset(w) + partial_bytes(rows, F, F);
}

extern "C" int avvad_stft_stats(const float* wave, const int* n_frames, double* acc, const avvad_stft_desc* d, void* wsv,
                                size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!wave || !n_frames || !acc || !wsv || ((uintptr_t)wsv & 15) || ((uintptr_t)acc & 7)) return AVVAD_EINVAL;
  const size_t need = avvad_stft_stats_workspace(d);
  if (!need) return AVVAD_EINVAL;
  if (ws_bytes < need) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  const int F = d->n_fft / 2 + 1;
  const long rows = (long)d->B * d->T;
  const frames::SpecWs w = frames::spec_ws(d->n_fft, rows);
  float* ws = (float*)wsv;
  double* part = (double*)((char*)wsv + partials_offset(w));
  int rc = frames::framed_dft(wave, d->L, d->B, d->T, d->n_fft, d->hop, ws, w, s);
  if (rc) return rc;
  launch_columns(SpectrumLogPower{ws + w.S, w.ld, d->eps}, rows, d->T, F, n_frames, part, s);
  launch_add(part, rows, F, F, n_frames, d->B, d->T, acc, s);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

extern "C" int avvad_stats_finalize(const double* acc, int nstat, float* mean, float* std_, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!acc || !mean || !std_ || nstat <= 0 || ((uintptr_t)acc & 7)) return AVVAD_EINVAL;
  hipLaunchKernelGGL(finalize, dim3((nstat + 255) / 256), dim3(256), 0, (hipStream_t)sv, acc, nstat, mean, std_);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
