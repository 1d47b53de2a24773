// scores.hip -- scores of the enhanced speech and of the classifier on the GPU: the scale-invariant energy ratios
// SI-SDR / SI-SIR / SI-SAR of a ragged batch of waveforms, and the confusion counts (tp, tn, fp, fn) of a ragged batch of
// frame labels.
//
// Replaces the host-side scoring of the reference:
//   packages/metrics.py:12-60            si_sdr_components (alpha_s, alpha_n, the three planes s_target / e_noise / e_art) and
//                                        energy_ratios (10 log10 of |s_target|^2 over |e_noise + e_art|^2, |e_noise|^2, |e_art|^2)
//   packages/models/utils.py:164-203     f1_loss's four sums tp / tn / fp / fn
//
// Energy ratios.  Every norm the reference takes is a quadratic form of six inner products of the estimate e, the clean
// reference r and the noise n (the Gram matrix of the three signals):
//   G = (e.e, e.r, e.n, r.r, n.n, r.n),   a_s = e.r / r.r,   a_n = e.n / n.n
//   |s_target|^2 = a_s e.r      |e_noise + e_art|^2 = e.e - a_s e.r      |e_noise|^2 = a_n e.n
//   |e_art|^2 = e.e - a_s e.r - a_n e.n + 2 a_s a_n r.n
// so ONE pass over the three signals (12 bytes per sample) is all the data traffic; the planes are never written.  Every
// value is widened to double before it is multiplied.  third_mode 2 reads the noisy mixture x and forms n = (double)x -
// (double)r itself.
//
// An accumulator is [B][6] doubles in caller-owned device memory; calls ADD to it, so an utterance may arrive in packets.
//
// Kernel forms (memory-bound, and at an utterance's size launch-bound):
//   gram_partials<MODE>: rows are cut into chunks of AVVAD_SCORE_CHUNK samples; workgroup (chunk, row) has four waves whose
//        256 lanes stride over the chunk (a wave reads 256 consecutive bytes per signal and load, UN samples of each signal
//        in flight per lane: plain dword loads, since the three row bases are only 4-byte aligned and differently so);
//        cross-lane sums by a fixed butterfly, the four waves added in wave order (reduce.h); the workgroup stores one
//        6-double partial.  A workgroup whose chunk lies past the row's length exits and stores nothing.
//   gram_add: acc[row][c] += the row's partials in ascending chunk order (lane c < 6 of one wave per row); only the
//        chunks below the row's length are read.
//   gram_finalize: one thread per row, acc -> the three ratios in dB (and the two alpha).
//   sisdr_coefficients, sisdr_gradient (avvad_si_sdr_loss, training): gram_partials<0> and gram_add as above into a zeroed
//        accumulator of the workspace, then one workgroup turns each row's three sums into SI-SDR and the two coefficients
//        of its gradient (double, rounded once) and sums the loss in ascending row order; the gradient c1 ref + c2 est is
//        one pass on gram_partials' grid (chunk, row), exact zeros behind the row's length.
//   confusion_partials: workgroup (chunk of the row's len * Y values, row) counts in integers and adds its four counts to
//        counts[row][0..3] with 64-bit integer atomics (exact in any order: no workspace).
// No floating-point atomics, and the chunking depends on the row length alone: bit-identical run to run and whatever the
// CU cap.  Nothing at or behind lengths[b] (clamped to [0, L]) is read.
#include <math.h>

#include "reduce.h"

namespace {

constexpr int CHUNK = AVVAD_SCORE_CHUNK;   // samples of one partial
constexpr int UN = 8;                      // samples of each signal in flight per lane (measured: tools/lab/score_lab.hip)
constexpr int CONF_CHUNK = 4096;           // values of one confusion workgroup
static_assert(CHUNK % (256 * UN) == 0, "a chunk is a whole number of unrolled workgroup strides");

// part[row][chunk][6], chunk < nchunks(L).  MODE 0: no third signal (its three products stay 0), 1: noise, 2: mixture.
template <int MODE>
__global__ void __launch_bounds__(256)
    gram_partials(const float* __restrict__ est, long ld_est, const float* __restrict__ ref, long ld_ref,
                  const float* __restrict__ third, long ld_third, const int* __restrict__ lengths, long L,
                  double* __restrict__ part) {
  __shared__ double red[6][4];
  const int b = blockIdx.y;
  const long len = row_len(lengths, b, L);
  const long i0 = (long)blockIdx.x * CHUNK;
  if (i0 >= len) return;                  // (uniform for the workgroup: nothing is waiting at the barrier below)
  const long i1 = min(len, i0 + CHUNK);
  const float* e = est + b * ld_est;
  const float* r = ref + b * ld_ref;
  const float* t = MODE ? third + b * ld_third : nullptr;
  double g[6] = {};
  for (long i = i0 + threadIdx.x; i < i1; i += 256 * UN) {
    float ve[UN] = {}, vr[UN] = {}, vt[UN] = {};
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const long j = i + u * 256;
      if (j < i1) {
        ve[u] = e[j], vr[u] = r[j];
        if (MODE) vt[u] = t[j];
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {         // (a lane past the end adds exact zeros)
      const double de = (double)ve[u], dr = (double)vr[u];
      g[0] += de * de;
      g[1] += de * dr;
      g[3] += dr * dr;
      if (MODE) {
        const double dn = MODE == 2 ? (double)vt[u] - dr : (double)vt[u];
        g[2] += de * dn;
        g[4] += dn * dn;
        g[5] += dr * dn;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) fold4_put(red[c], g[c], Add());
  __syncthreads();
  if (threadIdx.x < 6) {
    const int c = threadIdx.x;
    part[((long)b * gridDim.x + blockIdx.x) * 6 + c] = fold4_get(red[c], Add());
  }
}

// acc[row][c] += partials of the chunks below the row's length, ascending
__global__ void __launch_bounds__(64)
    gram_add(const double* __restrict__ part, int nchunks, const int* __restrict__ lengths, long L, double* __restrict__ acc) {
  const int b = blockIdx.x, c = threadIdx.x;
  if (c >= 6) return;
  const long len = row_len(lengths, b, L);
  const int n = (int)chunks_of(len, CHUNK);            // <= nchunks
  const double* p = part + (long)b * nchunks * 6 + c;
  acc[b * 6 + c] = add_ascending<8>(acc[b * 6 + c], p, 6, 0, n);
}

// 10 log10(num / den) with the reference's IEEE behaviour: den == 0 gives inf (0 / 0: NaN), and a den that cancellation
// drove slightly negative counts as 0 (stats.hip's variance clamp); a NaN den stays a NaN
__device__ __forceinline__ double ratio_db(double num, double den) {
  if (den < 0.0) den = 0.0;
  return 10.0 * log10(num / den);
}

__global__ void gram_finalize(const double* __restrict__ acc, int B, int mode, double* __restrict__ ratios,
                              double* __restrict__ alpha) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* g = acc + (long)b * 6;
  const double ee = g[0], er = g[1], en = g[2], rr = g[3], nn = g[4], rn = g[5];
  const double nan = __builtin_nan("");
  const double a_s = er / rr;              // an empty row: 0 / 0
  const double target = a_s * er;
  const double a_n = mode ? en / nn : nan;
  const double noise = a_n * en;
  ratios[b * 3 + 0] = ratio_db(target, ee - target);
  ratios[b * 3 + 1] = mode ? ratio_db(target, noise) : nan;
  ratios[b * 3 + 2] = mode ? ratio_db(target, ee - target - noise + 2.0 * a_s * a_n * rn) : nan;
  if (alpha) alpha[b * 2 + 0] = a_s, alpha[b * 2 + 1] = a_n;
}

// counts[row] += (tp, tn, fp, fn) over the row's first len * Y values; a value is "1" when > 0.5 (logits: > 0)
__global__ void __launch_bounds__(256)
    confusion_partials(const float* __restrict__ pred, int logits, const float* __restrict__ target,
                       const int* __restrict__ lengths, int T, int Y, unsigned long long* __restrict__ counts) {
  __shared__ int red[4][4];
  const int b = blockIdx.y;
  const long n = (long)row_count(lengths, b, T) * Y;
  const long i0 = (long)blockIdx.x * CONF_CHUNK;
  if (i0 >= n) return;
  const long i1 = min(n, i0 + CONF_CHUNK);
  const float* p = pred + (long)b * T * Y;
  const float* y = target + (long)b * T * Y;
  const float thr = logits ? 0.f : 0.5f;
  int c[4] = {};
  for (long i = i0 + threadIdx.x; i < i1; i += 256) {
    const int hp = p[i] > thr, hy = y[i] > 0.5f;
    c[0] += hp & hy;
    c[1] += (hp | hy) ^ 1;
    c[2] += hp & (hy ^ 1);
    c[3] += (hp ^ 1) & hy;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) fold4_put(red[k], c[k], Add());
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    const int v = fold4_get(red[k], Add());
    if (v) atomicAdd(counts + (long)b * 4 + k, (unsigned long long)v);
  }
}

// ---- the SI-SDR loss (avvad_si_sdr_loss): gram_partials<0> / gram_add's sums, then two coefficients per row and one pass
__global__ void zero_doubles(double* __restrict__ p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0.0;
}

// One workgroup.  Per row, with a = e.r, r = r.r, e = e.e, P = a^2 / r, D = e - P: sdr[b] = gram_finalize's SI-SDR, and the
// gradient of -SI-SDR in the estimate is c1 ref + c2 est, c2 = (20 / ln 10) / D, c1 = -(20 / ln 10) (1 / a + a / (r D)),
// formed in double and rounded once each.  A row with an empty window: sdr NaN (as gram_finalize), coefficients 0, nothing
// added to the loss.  loss = -(sum_b sdr[b]) in ascending row order by one thread.
__global__ void __launch_bounds__(256)
    sisdr_coefficients(const double* __restrict__ acc, const int* __restrict__ lengths, long L, int B, double* __restrict__ sdr,
                       double* __restrict__ ratios, float* __restrict__ coef, float* __restrict__ loss) {
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const long len = row_len(lengths, b, L);
    const double ee = acc[b * 6 + 0], er = acc[b * 6 + 1], rr = acc[b * 6 + 3];
    const double target = (er / rr) * er, D = ee - target;
    const double k = 20.0 / log(10.0);
    const double v = ratio_db(target, D);
    sdr[b] = v;
    if (ratios) ratios[b] = v;
    coef[2 * b + 0] = len > 0 ? (float)(-k * (1.0 / er + er / (rr * D))) : 0.f;
    coef[2 * b + 1] = len > 0 ? (float)(k / D) : 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int b = 0; b < B; ++b)
      if (!lengths || lengths[b] > 0) sum += sdr[b];
    loss[0] = (float)-sum;
  }
}

// dest[b][i] = c1[b] ref[b][i] + c2[b] est[b][i] below the row's length, exact zeros from there to L; the grid of
// gram_partials (chunk, row).  Nothing of est / ref at or behind the length is read.
__global__ void __launch_bounds__(256)
    sisdr_gradient(const float* __restrict__ est, long ld_est, const float* __restrict__ ref, long ld_ref,
                   const int* __restrict__ lengths, long L, const float* __restrict__ coef, float* __restrict__ dest, long ld_dest) {
  const int b = blockIdx.y;
  const long len = row_len(lengths, b, L);
  const long i0 = (long)blockIdx.x * CHUNK, i1 = min(L, i0 + CHUNK);
  const float c1 = coef[2 * b], c2 = coef[2 * b + 1];
  const float* e = est + b * ld_est;
  const float* r = ref + b * ld_ref;
  float* d = dest + b * ld_dest;
  for (long i = i0 + threadIdx.x; i < i1; i += 256) d[i] = i < len ? c1 * r[i] + c2 * e[i] : 0.f;
}

inline long n_chunks(long L) { return chunks_of(L, CHUNK); }
inline bool ok_shape(int B, long L) {
  return B > 0 && B <= 65535 && L > 0 && L < (1L << 40) && n_chunks(L) * B < (1L << 31) / 6;
}
inline size_t partial_bytes(int B, long L) { return align_up((size_t)B * n_chunks(L) * 6 * sizeof(double), 256); }

template <int MODE>
void launch_partials(const float* est, long ld_est, const float* ref, long ld_ref, const float* third, long ld_third,
                     const int* lengths, int B, long L, double* part, hipStream_t s) {
  hipLaunchKernelGGL(gram_partials<MODE>, dim3((unsigned)n_chunks(L), B), dim3(256), 0, s, est, ld_est, ref, ld_ref, third,
                     ld_third, lengths, L, part);
}

// workspace of the loss: [partials][acc B x 6 doubles][sdr B doubles][coef B x 2 floats], byte offsets
struct LossWs { size_t acc, sdr, coef, total; };
inline LossWs loss_ws(int B, long L) {
  LossWs w;
  w.acc = partial_bytes(B, L);
  w.sdr = w.acc + align_up((size_t)B * 6 * sizeof(double), 256);
  w.coef = w.sdr + align_up((size_t)B * sizeof(double), 256);
  w.total = w.coef + align_up((size_t)B * 2 * sizeof(float), 256);
  return w;
}

}  // namespace

extern "C" size_t avvad_score_workspace(int B, long L) { return ok_shape(B, L) ? partial_bytes(B, L) : 0; }

extern "C" int avvad_score_accumulate(const float* est, long ld_est, const float* ref, long ld_ref, const float* third,
                                      long ld_third, int third_mode, const int* lengths, double* acc, int B, long L, void* ws,
                                      size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!est || !ref || !acc || !ws || third_mode < 0 || third_mode > 2 || (third_mode != 0) != (third != nullptr)) return AVVAD_EINVAL;
  if (!ok_shape(B, L) || ld_est < L || ld_ref < L || (third_mode && ld_third < L)) return AVVAD_EINVAL;
  if (((uintptr_t)ws & 255) || ((uintptr_t)acc & 7)) return AVVAD_EINVAL;
  if (ws_bytes < partial_bytes(B, L)) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  double* part = (double*)ws;
  if (third_mode == 0) launch_partials<0>(est, ld_est, ref, ld_ref, third, ld_third, lengths, B, L, part, s);
  else if (third_mode == 1) launch_partials<1>(est, ld_est, ref, ld_ref, third, ld_third, lengths, B, L, part, s);
  else launch_partials<2>(est, ld_est, ref, ld_ref, third, ld_third, lengths, B, L, part, s);
  hipLaunchKernelGGL(gram_add, dim3(B), dim3(64), 0, s, part, (int)n_chunks(L), lengths, L, acc);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

extern "C" int avvad_score_finalize(const double* acc, int B, int third_mode, double* ratios, double* alpha, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!acc || !ratios || B <= 0 || third_mode < 0 || third_mode > 2) return AVVAD_EINVAL;
  if (((uintptr_t)acc & 7) || ((uintptr_t)ratios & 7) || ((uintptr_t)alpha & 7)) return AVVAD_EINVAL;
  hipLaunchKernelGGL(gram_finalize, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)sv, acc, B, third_mode, ratios, alpha);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

extern "C" int avvad_confusion_accumulate(const float* pred, int pred_mode, const float* target, const int* lengths,
                                          long long* counts, int B, int T, int Y, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!pred || !target || !counts || pred_mode < 0 || pred_mode > 1 || B <= 0 || B > 65535 || T <= 0 || Y <= 0) return AVVAD_EINVAL;
  const long chunks = chunks_of((long)T * Y, CONF_CHUNK);
  if (chunks >= (1L << 31) || ((uintptr_t)counts & 7)) return AVVAD_EINVAL;
  hipLaunchKernelGGL(confusion_partials, dim3((unsigned)chunks, B), dim3(256), 0, (hipStream_t)sv, pred, pred_mode, target, lengths,
                     T, Y, (unsigned long long*)counts);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

extern "C" size_t avvad_si_sdr_loss_workspace(int B, long L) { return ok_shape(B, L) ? loss_ws(B, L).total : 0; }

extern "C" int avvad_si_sdr_loss(const float* est, long ld_est, const float* ref, long ld_ref, const int* lengths, float* loss,
                                 double* ratios, float* dest, long ld_dest, int B, long L, void* ws, size_t ws_bytes,
                                 avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!est || !ref || !loss || !dest || !ws || !ok_shape(B, L) || ld_est < L || ld_ref < L || ld_dest < L) return AVVAD_EINVAL;
  if (ws_misaligned(ws) || ((uintptr_t)ratios & 7)) return AVVAD_EINVAL;
  const LossWs w = loss_ws(B, L);
  if (ws_bytes < w.total) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  double* part = (double*)ws;
  double* acc = (double*)((char*)ws + w.acc);
  double* sdr = (double*)((char*)ws + w.sdr);
  float* coef = (float*)((char*)ws + w.coef);
  hipLaunchKernelGGL(zero_doubles, dim3((B * 6 + 255) / 256), dim3(256), 0, s, acc, B * 6);
  launch_partials<0>(est, ld_est, ref, ld_ref, nullptr, 0, lengths, B, L, part, s);
  hipLaunchKernelGGL(gram_add, dim3(B), dim3(64), 0, s, part, (int)n_chunks(L), lengths, L, acc);
  hipLaunchKernelGGL(sisdr_coefficients, dim3(1), dim3(256), 0, s, acc, lengths, L, B, sdr, ratios, coef, loss);
  hipLaunchKernelGGL(sisdr_gradient, dim3((unsigned)n_chunks(L), B), dim3(256), 0, s, est, ld_est, ref, ld_ref, lengths, L, coef,
                     dest, ld_dest);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
