// stoi.hip -- intelligibility scores of the enhanced speech on the GPU: STOI (Taal et al. 2011) and its extended form
// ESTOI (Jensen & Taal 2016) of a ragged batch of (clean, processed) waveform pairs.
//
// Replaces: nothing the reference has -- its papers report the two scores from a host-side Python package.  The definition
// is include/avvad.h's (avvad_stoi) and tests/stoi_ref.py restates it in float64, stage by stage.
//
// Passes (every constant is fixed: 10 kHz, frames of 256 at hop 128, 512-point DFT, 15 third-octave bands, 30-frame segments):
//   resample     fs 16000 only.  Polyphase 5/8 with the caller's 161 double taps: one output sample per thread, its 32 or 33
//                products widened to double, summed in tap order, rounded once to float32.  Both signals, grid (chunk, row, signal).
//   keep_frames  one workgroup of 16 waves per row.  The clean row's frame energies in double (a wave per frame: four samples per lane in
//                sample order, the fixed butterfly of reduce.h), e = 20 log10(|w x| + eps) to the workspace; the row maximum (a NaN
//                propagates, as numpy.max has it); keep flags (max - 40) - e < 0 and their exclusive scan by wave ballots into
//                the kept-frame list; info = (frames, kept, segments).
//   overlap_add  x_sil / y_sil materialised: sample j is the sum, in double and in frame order, of the one or two kept
//                windowed frames that cover it, rounded once; exact zeros behind the row's own end.
//   banded_dft   (frames.h) the 256-sample frames of x_sil / y_sil under the symmetric Hann as ONE fp32-MFMA product against
//                the 256 x 424 basis of bins 7 .. 218 of a 512-point DFT.
//   band_norms   one thread per (frame, band): sum of re^2 + im^2 over the band's bins in bin order, widened to double, sqrt.
//   segments     one wave per (row, segment) on the 15 x 30 block in LDS, all in double: STOI's clipped, normalised row
//                correlations (lane = band) and ESTOI's row-then-column normalisation (lane = band, then lane = frame);
//                per-segment partials to the workspace.
//   finalize     one thread per row: the partials in ascending segment order, d = sum / (15 S) and sum / S; a row with fewer
//                than 30 frames after removal scores 1e-5.
// No floating-point atomics; every sum has a fixed order that depends on the row alone; the product is scheduled in whole
// tiles (an ordered fmaf chain per value), so a row's bits do not depend on its batch, on the CU cap or on the run.
// Nothing at or behind lengths[b] (clamped to [0, L]) is read.
//
// The training loss (avvad_stoi_loss) runs the same passes, then their adjoints in the processed signal, stage by stage,
// every one a gather with fixed-order double sums (the keep decision and the kept-frame list are constants of the backward):
//   segments_grad     one wave per (row, segment): the gradient of -d in the segment's 15 x 30 block of processed band
//                     magnitudes -- STOI through the strictly unclipped elements and through alpha, ESTOI through the two
//                     unit maps in reverse -- to a block of its own in the workspace.
//   band_grad         one thread per (frame, band): the blocks of the up to 30 segments that hold the frame, in ascending
//                     segment order; dS = dY S / Y (0 where Y is 0) over the band's bins, rounded to the float32 operand of
//   banded_dft_adjoint  (frames.h) dframes = dS . basis^T, ONE fp32-MFMA product in whole tiles.
//   invert_kept       frame -> position in the kept list, or -1.
//   ola_adjoint       one thread per 10 kHz sample: the one or two kept frames that cover it, each through the one or two
//                     frames of the second framing, under the window, in double; float32 at fs 10000, else kept as doubles for
//   resample_adjoint  one thread per 16 kHz sample: its about 20 taps in ascending output order, in double, rounded once.
//   loss_sum          one thread: -sum_b d_b in ascending row order, rounded once.
#include <math.h>

#include "frames.h"
#include "reduce.h"

namespace {

constexpr int FRAME = 256, HOP = 128, NFFT = 512, F0 = 7, NBIN = 212, NBAND = 15, SEG = 30, NTAP = 161, HALF = 80;
constexpr int UP = 5, DOWN = 8;
constexpr double EPS = 2.220446049250313e-16;      // 2^-52
constexpr double DYN_RANGE = 40.0;
constexpr double DEGENERATE = 1e-5;                // score of a row without a segment
// first bin of band j (and, at j = 15, the end of the last band): the bins nearest 150 * 2^((2j - 1) / 6) Hz on the grid k * 10000 / 512
__device__ const int BAND_EDGE[NBAND + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
static_assert(F0 + NBIN == 219, "bins 7 .. 218");

// numpy.minimum: a NaN on either side propagates
__device__ __forceinline__ double min_nan(double a, double b) { return (a != a || b != b) ? a + b : (a < b ? a : b); }

__host__ __device__ inline long resampled(long len) { return (UP * len + DOWN - 1) / DOWN; }
__host__ __device__ inline long frame_count(long len) { return len > FRAME ? (len - FRAME + HOP - 1) / HOP : 0; }   // starts i < len - 256
// samples of row b in the 10 kHz domain
__device__ __forceinline__ long row_len_10k(const int* lengths, int b, long L, int rate16) {
  const long len = row_len(lengths, b, L);
  return rate16 ? resampled(len) : len;
}
__device__ __forceinline__ int segments_of(int kept) {
  const int M = kept > 0 ? kept - 1 : 0;
  return M >= SEG ? M - SEG + 1 : 0;
}

// out[(sig, b)][n] = sum_t taps[t] xup[8 n + 80 - t], xup[5 m] = x[m]: scipy.signal.resample_poly(x, 5, 8)'s centring
__global__ void __launch_bounds__(256)
    resample(const float* __restrict__ x, long ldx, const float* __restrict__ y, long ldy, const int* __restrict__ lengths, long L,
             const double* __restrict__ taps, float* __restrict__ out, long ld_out) {
  const int b = blockIdx.y, sig = blockIdx.z;
  const long len = row_len(lengths, b, L);
  const long n = (long)blockIdx.x * 256 + threadIdx.x;
  if (n >= resampled(len)) return;
  const float* src = sig ? y + b * ldy : x + b * ldx;
  const long c = DOWN * n + HALF;
  double acc = 0.0;
  for (int t = (int)(c % UP); t < NTAP; t += UP) {
    const long m = (c - t) / UP;
    if (m >= 0 && m < len) acc += taps[t] * (double)src[m];
  }
  out[((long)sig * gridDim.y + b) * ld_out + n] = (float)acc;
}

// one workgroup of KEEP_WAVES waves per row of the clean signal x [B][ldx]; en [B][nf_p], idx [B][nf_p], nk [B], info [B][3]
constexpr int KEEP_WAVES = 16, KEEP_THREADS = 64 * KEEP_WAVES;
__global__ void __launch_bounds__(KEEP_THREADS)
    keep_frames(const float* __restrict__ x, long ldx, const int* __restrict__ lengths, long L, int rate16, double* __restrict__ en,
                int* __restrict__ idx, int nf_p, int* __restrict__ nk, int* __restrict__ info) {
  __shared__ double w[FRAME];
  __shared__ double wmax[KEEP_WAVES];
  __shared__ int wnan[KEEP_WAVES], wcnt[KEEP_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nf = (int)frame_count(row_len_10k(lengths, b, L, rate16));
  const float* xr = x + b * ldx;
  double* e = en + (long)b * nf_p;
  int* ix = idx + (long)b * nf_p;
  if (tid < FRAME) w[tid] = frames::hann_sym(tid, FRAME);
  __syncthreads();
  for (int i = wv; i < nf; i += KEEP_WAVES) {
    const float* f = xr + (long)i * HOP;
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = lane + 64 * u;
      const double v = w[k] * (double)f[k];
      s += v * v;
    }
    s = wave_sum(s);
    if (lane == 0) e[i] = 20.0 * log10(sqrt(s) + EPS);
  }
  __syncthreads();
  double m = -INFINITY;
  int nan = 0;
  for (int i = tid; i < nf; i += KEEP_THREADS) {
    const double v = e[i];
    if (v != v) nan = 1;
    else m = v > m ? v : m;
  }
  m = wave_fold(m, [](double m, double t) { return t > m ? t : m; });
  nan = __any(nan);
  if (lane == 0) wmax[wv] = m, wnan[wv] = nan;
  __syncthreads();
  nan = 0;
  for (int k = 0; k < KEEP_WAVES; ++k) {
    m = wmax[k] > m ? wmax[k] : m;
    nan |= wnan[k];
  }
  const double thr = nan ? __builtin_nan("") : m - DYN_RANGE;
  int base = 0;
  for (int i0 = 0; i0 < nf; i0 += KEEP_THREADS) {
    const int i = i0 + tid;
    const bool keep = i < nf && (thr - e[i] < 0.0);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wcnt[wv] = __popcll(mask);
    __syncthreads();
    int off = base;
    for (int k = 0; k < KEEP_WAVES; ++k) {
      if (k == wv) off = base;
      base += wcnt[k];
    }
    if (keep) ix[off + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    __syncthreads();
  }
  if (tid == 0) {
    nk[b] = base;
    info[b * 3 + 0] = nf;
    info[b * 3 + 1] = base;
    info[b * 3 + 2] = segments_of(base);
  }
}

// sil[(sig, b)][j] = the kept windowed frames overlap-added at hop 128; grid (chunk of ld_sil, row, signal)
__global__ void __launch_bounds__(256)
    overlap_add(const float* __restrict__ x, long ldx, const float* __restrict__ y, long ldy, const int* __restrict__ idx, int nf_p,
                int nf, const int* __restrict__ nk, float* __restrict__ sil, long ld_sil) {
  __shared__ double w[FRAME];
  const int b = blockIdx.y, sig = blockIdx.z;
  w[threadIdx.x] = frames::hann_sym(threadIdx.x, FRAME);
  __syncthreads();
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= ld_sil) return;
  const float* src = sig ? y + b * ldy : x + b * ldx;
  const int* ix = idx + (long)b * nf_p;
  const int n = clamp_count(nk[b], nf);         // (nf: the most frames a row of this call has, so every read stays in its row)
  const long q = j / HOP;
  const int r = (int)(j - q * HOP);
  double v = 0.0;
  if (q >= 1 && q - 1 < n) v += w[r + HOP] * (double)src[(long)clamp_count(ix[q - 1], nf - 1) * HOP + r + HOP];
  if (q < n) v += w[r] * (double)src[(long)clamp_count(ix[q], nf - 1) * HOP + r];
  sil[((long)sig * gridDim.y + b) * ld_sil + j] = (float)v;
}

// band[m][j] = sqrt(sum over the band's bins of re^2 + im^2), m over all frames of all rows of both signals
__global__ void __launch_bounds__(256) band_norms(const float* __restrict__ S, int ld, long n_frames, double* __restrict__ band) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_frames * NBAND) return;
  const long m = i / NBAND;
  const int j = (int)(i - m * NBAND);
  const float* row = S + m * ld;
  double s = 0.0;
  for (int f = BAND_EDGE[j]; f < BAND_EDGE[j + 1]; ++f) {
    const float2 c = *reinterpret_cast<const float2*>(row + 2 * (f - F0));
    s += (double)c.x * (double)c.x + (double)c.y * (double)c.y;
  }
  band[i] = sqrt(s);
}

// v[0 .. n) (stride st) -> (v - mean) / (|v - mean| + eps) in place, sums in index order
__device__ __forceinline__ void normalise(double* v, int n, int st) {
  double mean = 0.0;
  for (int t = 0; t < n; ++t) mean += v[t * st];
  mean /= (double)n;
  double ss = 0.0;
  for (int t = 0; t < n; ++t) {
    const double c = v[t * st] - mean;
    v[t * st] = c;
    ss += c * c;
  }
  const double inv = sqrt(ss) + EPS;
  for (int t = 0; t < n; ++t) v[t * st] /= inv;
}

// one wave per (segment, row); band [2][B][mf][15]; part [B][ns][2] = (sum over the bands of STOI's correlations, ESTOI's sum / 30)
__global__ void __launch_bounds__(64)
    segments(const double* __restrict__ band, const int* __restrict__ nk, int B, int mf, int ns, int which, double* __restrict__ part) {
  constexpr int LD = SEG + 1;
  __shared__ double X[NBAND * LD], Y[NBAND * LD], P[NBAND * LD], red[SEG];
  const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  if (s >= segments_of(clamp_count(nk[b], mf + 1))) return;      // (uniform: nobody waits at a barrier below)
  for (int e = tid; e < NBAND * SEG; e += 64) {
    const int t = e / NBAND, j = e - t * NBAND;
    X[j * LD + t] = band[((long)b * mf + s + t) * NBAND + j];
    Y[j * LD + t] = band[(((long)B + b) * mf + s + t) * NBAND + j];
  }
  __syncthreads();
  double stoi = 0.0, estoi = 0.0;
  if (which & 1) {
    if (tid < NBAND) {
      const double *x = X + tid * LD, *y = Y + tid * LD;
      double *p = P + tid * LD;
      double nx = 0.0, ny = 0.0;
      for (int t = 0; t < SEG; ++t) nx += x[t] * x[t], ny += y[t] * y[t];
      const double alpha = sqrt(nx) / (sqrt(ny) + EPS);
      const double clip = 1.0 + 5.623413251903491;             // 1 + 10^(15 / 20)
      double mx = 0.0, mp = 0.0;
      for (int t = 0; t < SEG; ++t) {
        p[t] = min_nan(alpha * y[t], x[t] * clip);
        mx += x[t], mp += p[t];
      }
      mx /= (double)SEG, mp /= (double)SEG;
      double sx = 0.0, sp = 0.0, sxp = 0.0;
      for (int t = 0; t < SEG; ++t) {
        const double cx = x[t] - mx, cp = p[t] - mp;
        sx += cx * cx, sp += cp * cp;
      }
      const double ix = sqrt(sx) + EPS, ip = sqrt(sp) + EPS;
      for (int t = 0; t < SEG; ++t) sxp += ((x[t] - mx) / ix) * ((p[t] - mp) / ip);
      red[tid] = sxp;
    }
    __syncthreads();
    if (tid == 0)
      for (int j = 0; j < NBAND; ++j) stoi += red[j];
    __syncthreads();
  }
  if (which & 2) {
    if (tid < NBAND) normalise(X + tid * LD, SEG, 1), normalise(Y + tid * LD, SEG, 1);
    __syncthreads();
    if (tid < SEG) {
      normalise(X + tid, NBAND, LD), normalise(Y + tid, NBAND, LD);
      double c = 0.0;
      for (int j = 0; j < NBAND; ++j) c += X[j * LD + tid] * Y[j * LD + tid];
      red[tid] = c;
    }
    __syncthreads();
    if (tid == 0) {
      for (int t = 0; t < SEG; ++t) estoi += red[t];
      estoi /= (double)SEG;
    }
  }
  if (tid == 0) part[((long)b * ns + s) * 2 + 0] = stoi, part[((long)b * ns + s) * 2 + 1] = estoi;
}

// d[b] = (STOI, ESTOI); a score that was not asked for is NaN
__global__ void finalize(const double* __restrict__ part, const int* __restrict__ nk, int B, int mf, int ns, int which,
                         double* __restrict__ d) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = segments_of(clamp_count(nk[b], mf + 1));
  double s0 = 0.0, s1 = 0.0;
  const double* p = part + (long)b * ns * 2;
  int s = 0;
  for (; s + 8 <= n; s += 8) {                 // eight segments' loads in flight, added in segment order
    double2 t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = *reinterpret_cast<const double2*>(p + 2 * (s + u));
#pragma unroll
    for (int u = 0; u < 8; ++u) s0 += t[u].x, s1 += t[u].y;
  }
  for (; s < n; ++s) s0 += p[2 * s], s1 += p[2 * s + 1];
  const double nan = __builtin_nan("");
  d[b * 2 + 0] = (which & 1) ? (n ? s0 / ((double)NBAND * n) : DEGENERATE) : nan;
  d[b * 2 + 1] = (which & 2) ? (n ? s1 / (double)n : DEGENERATE) : nan;
}

// ---- the gradient of -d in the processed signal (avvad_stoi_loss)
// The adjoint of normalise(): v[0 .. n) (stride st) the map's input, g its output's cotangent, overwritten with the input's:
// c = v - mean, nn = |c|, dc = g / (nn + eps) - c (g.c) / (nn (nn + eps)^2) (the second term 0 when nn == 0), dv = dc - mean(dc)
__device__ __forceinline__ void unit_backward(const double* v, double* g, int n, int st) {
  double mean = 0.0;
  for (int t = 0; t < n; ++t) mean += v[t * st];
  mean /= (double)n;
  double ss = 0.0, gc = 0.0;
  for (int t = 0; t < n; ++t) {
    const double c = v[t * st] - mean;
    ss += c * c;
    gc += g[t * st] * c;
  }
  const double nn = sqrt(ss), inv = nn + EPS;
  const double k = nn != 0.0 ? gc / (nn * inv * inv) : 0.0;
  double md = 0.0;
  for (int t = 0; t < n; ++t) {
    const double dc = g[t * st] / inv - (nn != 0.0 ? (v[t * st] - mean) * k : 0.0);
    g[t * st] = dc;
    md += dc;
  }
  md /= (double)n;
  for (int t = 0; t < n; ++t) g[t * st] -= md;
}

// one wave per (segment, row), `which` 1 or 2; gblk [B][ns][15][30] = d(-d_b) / d(the segment's processed band magnitudes)
__global__ void __launch_bounds__(64)
    segments_grad(const double* __restrict__ band, const int* __restrict__ nk, int B, int mf, int ns, int which,
                  double* __restrict__ gblk) {
  constexpr int LD = SEG + 1;
  __shared__ double X[NBAND * LD], Y[NBAND * LD], P[NBAND * LD], G[NBAND * LD];
  const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  const int nseg = segments_of(clamp_count(nk[b], mf + 1));
  if (s >= nseg) return;                                           // (uniform: nobody waits at a barrier below)
  for (int e = tid; e < NBAND * SEG; e += 64) {
    const int t = e / NBAND, j = e - t * NBAND;
    X[j * LD + t] = band[((long)b * mf + s + t) * NBAND + j];
    Y[j * LD + t] = band[(((long)B + b) * mf + s + t) * NBAND + j];
  }
  __syncthreads();
  if (which == 1) {
    if (tid < NBAND) {
      const double *x = X + tid * LD, *y = Y + tid * LD;
      double *p = P + tid * LD, *g = G + tid * LD;
      double nx = 0.0, ny = 0.0;
      for (int t = 0; t < SEG; ++t) nx += x[t] * x[t], ny += y[t] * y[t];
      const double sqx = sqrt(nx), sqy = sqrt(ny);
      const double alpha = sqx / (sqy + EPS);
      const double clip = 1.0 + 5.623413251903491;             // 1 + 10^(15 / 20)
      double mx = 0.0;
      for (int t = 0; t < SEG; ++t) {
        p[t] = min_nan(alpha * y[t], x[t] * clip);
        mx += x[t];
      }
      mx /= (double)SEG;
      double sx = 0.0;
      for (int t = 0; t < SEG; ++t) sx += (x[t] - mx) * (x[t] - mx);
      const double ix = sqrt(sx) + EPS, scale = -1.0 / ((double)NBAND * nseg);
      for (int t = 0; t < SEG; ++t) g[t] = scale * ((x[t] - mx) / ix);
      unit_backward(p, g, SEG, 1);                             // g: the cotangent of p
      // the tie went to the clip branch (min_nan), so only alpha y < C x carries a gradient: directly, and through alpha
      double dot = 0.0;
      for (int t = 0; t < SEG; ++t)
        if (alpha * y[t] < x[t] * clip) dot += g[t] * y[t];
      const double k = sqy != 0.0 ? sqx / (sqy * (sqy + EPS) * (sqy + EPS)) * dot : 0.0;
      for (int t = 0; t < SEG; ++t) g[t] = (alpha * y[t] < x[t] * clip ? alpha * g[t] : 0.0) - (sqy != 0.0 ? k * y[t] : 0.0);
    }
  } else {
    if (tid < NBAND) {
      for (int t = 0; t < SEG; ++t) P[tid * LD + t] = Y[tid * LD + t];
      normalise(X + tid * LD, SEG, 1), normalise(P + tid * LD, SEG, 1);     // P: the rows normalised over time
    }
    __syncthreads();
    if (tid < SEG) {
      normalise(X + tid, NBAND, LD);
      const double scale = -1.0 / ((double)SEG * nseg);
      for (int j = 0; j < NBAND; ++j) G[j * LD + tid] = scale * X[j * LD + tid];
      unit_backward(P + tid, G + tid, NBAND, LD);              // over the bands ...
    }
    __syncthreads();
    if (tid < NBAND) unit_backward(Y + tid * LD, G + tid * LD, SEG, 1);    // ... then over time
  }
  __syncthreads();
  double* out = gblk + ((long)b * ns + s) * (NBAND * SEG);
  for (int e = tid; e < NBAND * SEG; e += 64) {
    const int j = e / SEG, t = e - j * SEG;
    out[e] = G[j * LD + t];
  }
}

// one thread per (row, frame, band): dY[m][j] = the blocks of segments max(0, m - 29) .. min(S - 1, m) in ascending order, then
// dS[m][2 (f - 7) + {re, im}] = dY S / Y over the band's bins (0 where Y == 0, and on frames no segment holds).
// S, band: the processed half of the forward's; dS [B mf][ld]
__global__ void __launch_bounds__(256)
    band_grad(const double* __restrict__ gblk, const float* __restrict__ S, const double* __restrict__ band, const int* __restrict__ nk,
              int B, int mf, int ns, int ld, float* __restrict__ dS) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * mf * NBAND) return;
  const long fr = i / NBAND;
  const int j = (int)(i - fr * NBAND), b = (int)(fr / mf), m = (int)(fr - (long)b * mf);
  const int kept = clamp_count(nk[b], mf + 1), nseg = segments_of(kept);
  double dy = 0.0, yv = 0.0;
  if (nseg > 0 && m < kept - 1) {
    const int s0 = m - (SEG - 1) > 0 ? m - (SEG - 1) : 0, s1 = m < nseg - 1 ? m : nseg - 1;
    for (int s = s0; s <= s1; ++s) dy += gblk[(((long)b * ns + s) * NBAND + j) * SEG + (m - s)];
    yv = band[(((long)B + b) * mf + m) * NBAND + j];
  }
  const float* src = S + (((long)B + b) * mf + m) * ld;
  float* dst = dS + fr * ld;
  for (int f = BAND_EDGE[j]; f < BAND_EDGE[j + 1]; ++f) {
    float2 o = make_float2(0.f, 0.f);
    if (yv != 0.0) {
      const float2 c = *reinterpret_cast<const float2*>(src + 2 * (f - F0));
      o = make_float2((float)(dy * (double)c.x / yv), (float)(dy * (double)c.y / yv));
    }
    *reinterpret_cast<float2*>(dst + 2 * (f - F0)) = o;
  }
}

// pos[b][f] = the position of frame f in row b's kept list (ascending, so a binary search), or -1; grid (chunk of nf_p, row)
__global__ void __launch_bounds__(256)
    invert_kept(const int* __restrict__ idx, int nf_p, int nf, const int* __restrict__ nk, int* __restrict__ pos) {
  const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf_p) return;
  const int* ix = idx + (long)b * nf_p;
  int lo = 0, hi = clamp_count(nk[b], nf);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ix[mid] < f) lo = mid + 1;
    else hi = mid;
  }
  pos[(long)b * nf_p + f] = (lo < clamp_count(nk[b], nf) && ix[lo] == f) ? lo : -1;
}

// The adjoints of the second framing, the kept-frame overlap-add and the first framing's window in one gather: sample i of
// the 10 kHz domain lies in frames i / 128 - 1 and i / 128; a kept one at position q put w[k] x[i] at sample 128 q + k of the
// overlap-added signal, which frames j - 1 and j (j = that sample / 128) of the second framing read (the second window is in the
// basis).  Up to four terms, in ascending frame order, in double; T = float writes the gradient itself (fs 10000), T = double
// the resampler adjoint's input.  Zeros at and behind the row's length, in rows without a segment and when !live.
// dfr [B][mf][256]; grid (chunk of ncols, row)
template <typename T>
__global__ void __launch_bounds__(256)
    ola_adjoint(const float* __restrict__ dfr, const int* __restrict__ pos, int nf_p, const int* __restrict__ nk,
                const int* __restrict__ lengths, long L, int rate16, int mf, int live, T* __restrict__ out, long ld_out, long ncols) {
  __shared__ double w[FRAME];
  w[threadIdx.x] = frames::hann_sym(threadIdx.x, FRAME);
  __syncthreads();
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= ncols) return;
  double v = 0.0;
  if (live) {
    const long len = row_len_10k(lengths, b, L, rate16);
    const long nfb = frame_count(len);
    const int kept = clamp_count(nk[b], mf + 1), M = kept > 0 ? kept - 1 : 0;
    if (i < len && segments_of(kept) > 0) {
      const float* d = dfr + (long)b * mf * FRAME;
      const int* ps = pos + (long)b * nf_p;
      // the cotangent of sample 128 q + k (k < 256) of the overlap-added signal
      auto dsil = [&](int q, int k) -> double {
        const int j = q + (k >= HOP ? 1 : 0), r = k >= HOP ? k - HOP : k;
        double s = 0.0;
        if (j >= 1 && j - 1 < M) s += (double)d[(long)(j - 1) * FRAME + r + HOP];
        if (j < M) s += (double)d[(long)j * FRAME + r];
        return s;
      };
      const long f = i / HOP;
      const int r = (int)(i - f * HOP);
      if (f >= 1 && f - 1 < nfb) {
        const int q = ps[f - 1];
        if (q >= 0 && q < kept) v += w[r + HOP] * dsil(q, r + HOP);
      }
      if (f < nfb) {
        const int q = ps[f];
        if (q >= 0 && q < kept) v += w[r] * dsil(q, r);
      }
    }
  }
  out[(long)b * ld_out + i] = (T)v;
}

// The adjoint of resample(): dproc[b][m] = sum_n taps[8 n + 80 - 5 m] dy[b][n] over the outputs n whose tap index lies in
// 0 .. 160, in ascending n, in double, rounded once; zeros at and behind the row's length and when !live.  grid (chunk of L, row)
__global__ void __launch_bounds__(256)
    resample_adjoint(const double* __restrict__ dy, long ld_dy, const int* __restrict__ lengths, long L, const double* __restrict__ taps,
                     int live, float* __restrict__ dproc, long ld) {
  const int b = blockIdx.y;
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= L) return;
  const long len = row_len(lengths, b, L);
  double acc = 0.0;
  if (live && m < len) {
    const long lo = UP * m - HALF, last = resampled(len) - 1;
    long n0 = lo > 0 ? (lo + DOWN - 1) / DOWN : 0, n1 = (UP * m + HALF) / DOWN;
    if (n1 > last) n1 = last;
    const double* row = dy + b * ld_dy;
    for (long n = n0; n <= n1; ++n) acc += taps[DOWN * n + HALF - UP * m] * row[n];
  }
  dproc[b * ld + m] = (float)acc;
}

// loss = -(sum_b d2[b][which - 1]) in ascending row order by one thread, rounded once; d[b] = the row's score
__global__ void __launch_bounds__(64) loss_sum(const double* __restrict__ d2, int B, int which, float* __restrict__ loss, double* __restrict__ d) {
  if (d)
    for (int b = threadIdx.x; b < B; b += 64) d[b] = d2[2 * b + which - 1];
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int b = 0; b < B; ++b) sum += d2[2 * b + which - 1];
    loss[0] = (float)-sum;
  }
}

// The workspace, byte offsets (each a multiple of 256): [rs 2 B x ld_rs floats, fs 16000 only][en B x nf_p doubles]
// [idx B x nf_p ints][nk B ints][sil 2 B x ld_sil floats][W 256 x ldS floats][S 2 B mf x ldS floats][band 2 B mf x 15 doubles]
// [part B x ns x 2 doubles]; everything behind nk only when a row can have a segment (mf >= 30)
struct Plan {
  int rate16, nf, nf_p, mf, ns, ldS;
  long Lr, ld_rs, ld_sil;
  size_t rs, en, idx, nk, sil, W, S, band, part, total;
};
inline bool plan(int B, long L, int fs, Plan& p) {
  if (B <= 0 || B > 32767 || L <= 0 || L > (1L << 30) || (fs != 16000 && fs != 10000)) return false;
  p.rate16 = fs == 16000;
  p.Lr = p.rate16 ? resampled(L) : L;
  p.nf = (int)frame_count(p.Lr);
  p.nf_p = (int)align_up((size_t)(p.nf > 0 ? p.nf : 1), 64);
  p.mf = p.nf > 0 ? p.nf - 1 : 0;
  p.ns = p.mf >= SEG ? p.mf - SEG + 1 : 0;
  p.ldS = frames::banded_ld(NBIN);
  p.ld_rs = (long)align_up((size_t)p.Lr, 64);
  p.ld_sil = (long)p.nf * HOP + HOP;                 // (nf - 1) 128 + 256: every frame kept
  if (p.ns > 0 && (double)2 * B * p.mf * p.ldS >= 2147483648.0) return false;
  size_t o = 0;
  p.rs = o, o += p.rate16 ? align_up((size_t)2 * B * p.ld_rs * sizeof(float), 256) : 0;
  p.en = o, o += align_up((size_t)B * p.nf_p * sizeof(double), 256);
  p.idx = o, o += align_up((size_t)B * p.nf_p * sizeof(int), 256);
  p.nk = o, o += align_up((size_t)B * sizeof(int), 256);
  p.sil = p.W = p.S = p.band = p.part = o;
  if (p.ns > 0) {
    p.sil = o, o += align_up((size_t)2 * B * p.ld_sil * sizeof(float), 256);
    p.W = o, o += align_up((size_t)FRAME * p.ldS * sizeof(float), 256);
    p.S = o, o += align_up((size_t)2 * B * p.mf * p.ldS * sizeof(float), 256);
    p.band = o, o += align_up((size_t)2 * B * p.mf * NBAND * sizeof(double), 256);
    p.part = o, o += align_up((size_t)B * p.ns * 2 * sizeof(double), 256);
  }
  p.total = o;
  return true;
}

// The loss's workspace: the forward's, then [pos B x nf_p ints][d2 B x 2 doubles][info B x 3 ints] and, when a row can have a
// segment, [gblk B x ns x 450 doubles][dfr B mf x 256 floats][dy10 B x ld_rs doubles, fs 16000 only].  dS takes the clean half
// of S, which band_norms has consumed by then.
struct LossPlan {
  Plan f;
  size_t pos, d2, info, gblk, dfr, dy10, total;
};
inline bool loss_plan(int B, long L, int fs, LossPlan& p) {
  if (!plan(B, L, fs, p.f)) return false;
  size_t o = p.f.total;
  p.pos = o, o += align_up((size_t)B * p.f.nf_p * sizeof(int), 256);
  p.d2 = o, o += align_up((size_t)B * 2 * sizeof(double), 256);
  p.info = o, o += align_up((size_t)B * 3 * sizeof(int), 256);
  p.gblk = p.dfr = p.dy10 = o;
  if (p.f.ns > 0) {
    p.gblk = o, o += align_up((size_t)B * p.f.ns * NBAND * SEG * sizeof(double), 256);
    p.dfr = o, o += align_up((size_t)B * p.f.mf * FRAME * sizeof(float), 256);
    p.dy10 = o, o += p.f.rate16 ? align_up((size_t)B * p.f.ld_rs * sizeof(double), 256) : 0;
  }
  p.total = o;
  return true;
}

// the forward passes of avvad_stoi within ws (carved by p); d [B][2], info [B][3]
int forward(const float* clean, long ld_clean, const float* proc, long ld_proc, const int* lengths, const double* taps, int B, long L,
            int which, double* d, int* info, char* ws, const Plan& p, hipStream_t s) {
  double* en = (double*)(ws + p.en);
  int* idx = (int*)(ws + p.idx);
  int* nk = (int*)(ws + p.nk);
  const float *x = clean, *y = proc;
  long ldx = ld_clean, ldy = ld_proc;
  if (p.rate16) {
    float* rs = (float*)(ws + p.rs);
    hipLaunchKernelGGL(resample, dim3(cdiv(p.Lr, 256), B, 2), dim3(256), 0, s, clean, ld_clean, proc, ld_proc, lengths, L, taps, rs,
                       p.ld_rs);
    x = rs, y = rs + (long)B * p.ld_rs, ldx = ldy = p.ld_rs;
  }
  hipLaunchKernelGGL(keep_frames, dim3(B), dim3(KEEP_THREADS), 0, s, x, ldx, lengths, L, p.rate16, en, idx, p.nf_p, nk, info);
  double* part = (double*)(ws + p.part);
  if (p.ns > 0) {
    float* sil = (float*)(ws + p.sil);
    float* S = (float*)(ws + p.S);
    double* band = (double*)(ws + p.band);
    hipLaunchKernelGGL(overlap_add, dim3(cdiv(p.ld_sil, 256), B, 2), dim3(256), 0, s, x, ldx, y, ldy, idx, p.nf_p, p.nf, nk, sil,
                       p.ld_sil);
    const int rc = frames::banded_dft(sil, p.ld_sil, 2 * B, p.mf, FRAME, NFFT, HOP, F0, NBIN, (float*)(ws + p.W), S, s);
    if (rc) return rc;
    const long n_frames = (long)2 * B * p.mf;
    hipLaunchKernelGGL(band_norms, dim3(cdiv(n_frames * NBAND, 256)), dim3(256), 0, s, S, p.ldS, n_frames, band);
    hipLaunchKernelGGL(segments, dim3(p.ns, B), dim3(64), 0, s, band, nk, B, p.mf, p.ns, which, part);
  }
  hipLaunchKernelGGL(finalize, dim3(cdiv(B, 64)), dim3(64), 0, s, part, nk, B, p.mf, p.ns, which, d);
  return AVVAD_OK;
}

}  // namespace

extern "C" size_t avvad_stoi_workspace(int B, long L, int fs) {
  Plan p;
  return plan(B, L, fs, p) ? p.total : 0;
}

extern "C" int avvad_stoi(const float* clean, long ld_clean, const float* proc, long ld_proc, const int* lengths, const double* taps,
                          int B, long L, int fs, int which, double* d, int* info, void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  Plan p;
  if (!clean || !proc || !d || !info || !wsv || which < 1 || which > 3 || !plan(B, L, fs, p)) return AVVAD_EINVAL;
  if (ld_clean < L || ld_proc < L || (p.rate16 && !taps)) return AVVAD_EINVAL;
  if (ws_misaligned(wsv) || ((uintptr_t)d & 7) || ((uintptr_t)taps & 7) || ((uintptr_t)info & 3)) return AVVAD_EINVAL;
  if (ws_bytes < p.total) return AVVAD_EWORKSPACE;
  const int rc = forward(clean, ld_clean, proc, ld_proc, lengths, taps, B, L, which, d, info, (char*)wsv, p, (hipStream_t)sv);
  if (rc) return rc;
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

extern "C" size_t avvad_stoi_loss_workspace(int B, long L, int fs) {
  LossPlan p;
  return loss_plan(B, L, fs, p) ? p.total : 0;
}

extern "C" int avvad_stoi_loss(const float* clean, long ld_clean, const float* proc, long ld_proc, const int* lengths, const double* taps,
                               int B, long L, int fs, int which, float* loss, double* d, int* info, float* dproc, long ld_dproc,
                               void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  LossPlan lp;
  if (!clean || !proc || !loss || !dproc || !wsv || which < 1 || which > 2 || !loss_plan(B, L, fs, lp)) return AVVAD_EINVAL;
  const Plan& p = lp.f;
  if (ld_clean < L || ld_proc < L || ld_dproc < L || (p.rate16 && !taps)) return AVVAD_EINVAL;
  if (ws_misaligned(wsv) || ((uintptr_t)d & 7) || ((uintptr_t)taps & 7) || ((uintptr_t)info & 3)) return AVVAD_EINVAL;
  if (ws_bytes < lp.total) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  char* ws = (char*)wsv;
  double* d2 = (double*)(ws + lp.d2);
  if (!info) info = (int*)(ws + lp.info);
  int rc = forward(clean, ld_clean, proc, ld_proc, lengths, taps, B, L, which, d2, info, ws, p, s);
  if (rc) return rc;
  hipLaunchKernelGGL(loss_sum, dim3(1), dim3(64), 0, s, d2, B, which, loss, d);
  const int* nk = (const int*)(ws + p.nk);
  int* pos = (int*)(ws + lp.pos);
  float* dfr = (float*)(ws + lp.dfr);
  const int live = p.ns > 0;
  if (live) {
    float* S = (float*)(ws + p.S);
    const double* band = (const double*)(ws + p.band);
    double* gblk = (double*)(ws + lp.gblk);
    float* dS = S;                                    // the clean half: consumed by band_norms
    hipLaunchKernelGGL(segments_grad, dim3(p.ns, B), dim3(64), 0, s, band, nk, B, p.mf, p.ns, which, gblk);
    hipLaunchKernelGGL(band_grad, dim3(cdiv((long)B * p.mf * NBAND, 256)), dim3(256), 0, s, gblk, S, band, nk, B, p.mf, p.ns, p.ldS, dS);
    rc = frames::banded_dft_adjoint(dS, B * p.mf, FRAME, NBIN, (const float*)(ws + p.W), dfr, s);
    if (rc) return rc;
    hipLaunchKernelGGL(invert_kept, dim3(cdiv(p.nf_p, 256), B), dim3(256), 0, s, (const int*)(ws + p.idx), p.nf_p, p.nf, nk, pos);
  }
  if (p.rate16) {
    double* dy10 = (double*)(ws + lp.dy10);
    if (live)
      hipLaunchKernelGGL(ola_adjoint<double>, dim3(cdiv(p.Lr, 256), B), dim3(256), 0, s, dfr, pos, p.nf_p, nk, lengths, L, 1, p.mf, 1,
                         dy10, p.ld_rs, p.Lr);
    hipLaunchKernelGGL(resample_adjoint, dim3(cdiv(L, 256), B), dim3(256), 0, s, dy10, p.ld_rs, lengths, L, taps, live, dproc, ld_dproc);
  } else {
    hipLaunchKernelGGL(ola_adjoint<float>, dim3(cdiv(L, 256), B), dim3(256), 0, s, dfr, pos, p.nf_p, nk, lengths, L, 0, p.mf, live,
                       dproc, ld_dproc, L);
  }
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
