// spectral_loss.hip -- the mask-regression training losses of a (B, T, F) mask head on the GPU, value and gradient in one
// grid-wide pass: mask MSE, signal approximation and spectrum approximation.
//
// Replaces: packages/models/utils.py:151-162 (mean_square_error_signal, mean_square_error_mask,
//   magnitude_spectrum_approxiamation_loss: a torch composition per utterance, the gradient from autograd's saved planes).
//
// With the mask m = pred (pred_mode 1) or sigmoid(pred) (pred_mode 2), the label y, the mixture's complex bin X and the
// clean speech's complex bin S, the term of cell (b, t, f) is
//   kind 0 (mask):      (y - m)^2
//   kind 1 (signal):    ((y - m) x)^2,  x = |X| = sqrtf(re^2 + im^2)
//   kind 2 (spectrum):  |S - m X|^2 = (Sr - m Xr)^2 + (Si - m Xi)^2
//   row_b = (1 / len_b) sum_{t < len_b} sum_f term,   loss = sum_b row_b,   dpred = d loss / d pred
// Terms and gradients are float32, sums double.  A row with len_b == 0 adds nothing and has a zero gradient.
//
// Kernel forms (memory-bound: pred, the label or the spectra are read once, dpred is written once):
//   spectral_pass<KIND, MODE>: a row's T * F cells, taken as one flat run, are cut into chunks of AVVAD_SPECTRAL_CHUNK
//        cells -- a function of (T, F) alone.  Workgroup (chunk, row) has four waves whose 256 lanes stride over the chunk,
//        UN cells in flight per lane.  pred / target / dpred are plain dword accesses (a wave touches 256 consecutive
//        bytes; F is odd, so a row of [T][F] floats is 16-byte aligned only by accident and nothing wider is assumed); a
//        complex bin is one 8-byte load through the spectrum's strides.  A lane finds (t, f) of its first cell by one
//        division and steps from there by 256 cells with a compare-and-subtract.  Cross-lane sum by a fixed butterfly,
//        the four waves added in wave order (reduce.h), one double partial per workgroup.  Cells at or behind len_b * F get an
//        exact zero gradient and nothing of the inputs there is read; a workgroup wholly behind them stores no partial.
//   spectral_finish: one workgroup; a wave per row adds the row's partials (only the chunks below the row's length) in a
//        fixed lane order and butterfly, divides by len_b in double; then one wave adds the rows the same way.
// No floating-point atomics, and the chunking never depends on B or the grid: bit-identical run to run, and a row's
// row_loss and dpred bits are the same alone and inside any batch.
#include <math.h>

#include "reduce.h"

namespace {

constexpr int CHUNK = AVVAD_SPECTRAL_CHUNK;   // cells of one partial
constexpr int UN = 4;                         // cells in flight per lane
static_assert(CHUNK % (256 * UN) == 0, "a chunk is a whole number of unrolled workgroup strides");

struct Spec { const float* p; long sb, st, sf; };

// part[row][chunk], chunk < nchunks(T * F)
template <int KIND, int MODE>
__global__ void __launch_bounds__(256)
    spectral_pass(const float* __restrict__ pred, const float* __restrict__ target, Spec X, Spec S,
                  const int* __restrict__ n_frames, int T, int F, double* __restrict__ part, float* dpred) {
  __shared__ double red[4];
  const int b = blockIdx.y;
  const int len = row_count(n_frames, b, T);
  const int n_row = T * F, n_valid = len * F;                // (< 2^30: launch precondition)
  const int i0 = blockIdx.x * CHUNK, i1 = min(n_row, i0 + CHUNK);
  const long base = (long)b * n_row;
  float* dq = dpred ? dpred + base : nullptr;
  if (i0 >= n_valid) {                    // (uniform) wholly behind the row's length: zeros, no partial
    if (dq)
      for (int j = i0 + threadIdx.x; j < i1; j += 256) dq[j] = 0.f;
    return;
  }
  const float* p = pred + base;
  const float* y = KIND < 2 ? target + base : nullptr;
  const float* xs = KIND >= 1 ? X.p + b * X.sb : nullptr;
  const float* ss = KIND == 2 ? S.p + b * S.sb : nullptr;
  const float inv = 1.f / (float)len;     // (len > 0 here)
  const int qs = 256 / F, rs = 256 % F;   // a step of 256 cells in (t, f)
  int t = (i0 + (int)threadIdx.x) / F, f = (i0 + (int)threadIdx.x) - t * F;
  double acc = 0.0;
  for (int j0 = i0 + threadIdx.x; j0 < i1; j0 += 256 * UN) {
    float pv[UN] = {}, yv[UN] = {};
    float2 xv[UN] = {}, sv[UN] = {};
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int j = j0 + u * 256;
      if (j < n_valid) {
        pv[u] = p[j];
        if (KIND < 2) yv[u] = y[j];
        if (KIND >= 1) xv[u] = *reinterpret_cast<const float2*>(xs + t * X.st + f * X.sf);
        if (KIND == 2) sv[u] = *reinterpret_cast<const float2*>(ss + t * S.st + f * S.sf);
      }
      t += qs, f += rs;
      if (f >= F) f -= F, ++t;
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int j = j0 + u * 256;
      const float m = MODE == 2 ? sigmoidf_(pv[u]) : pv[u];
      float term, g;
      if (KIND == 0) {
        const float d = yv[u] - m;
        term = d * d;
        g = -2.f * d;
      } else if (KIND == 1) {
        const float x = sqrtf(xv[u].x * xv[u].x + xv[u].y * xv[u].y);
        const float d = (yv[u] - m) * x;
        term = d * d;
        g = -2.f * d * x;
      } else {
        const float dr = sv[u].x - m * xv[u].x, di = sv[u].y - m * xv[u].y;
        term = dr * dr + di * di;
        g = -2.f * (dr * xv[u].x + di * xv[u].y);
      }
      if (MODE == 2) g *= m * (1.f - m);
      const bool valid = j < n_valid;
      acc += valid ? (double)term : 0.0;
      if (dq && j < i1) dq[j] = valid ? g * inv : 0.f;
    }
  }
  fold4_put(red, acc, Add());
  __syncthreads();
  if (threadIdx.x == 0) part[(long)b * gridDim.x + blockIdx.x] = fold4_get(red, Add());
}

// One workgroup of FIN_WAVES waves.  A wave per row (rows b = wave, wave + FIN_WAVES, ...): lane l adds the row's partials
// l, l + 64, ... in ascending order (only the chunks below the row's length), the 64 lane sums meet in the fixed
// butterfly, rows[b] = that / len_b, 0 for an empty row -- an order that depends on the row's chunk count alone.  Then
// wave 0 adds the rows the same way (lane l: rows l, l + 64, ...; the butterfly): an order that depends on B alone.
// (A single thread walking the partials and then the rows paid one memory round trip per value: 11.5 us at 16 x 76.)
constexpr int FIN_WAVES = 16;
__global__ void __launch_bounds__(64 * FIN_WAVES)
    spectral_finish(const double* __restrict__ part, int nchunks, const int* __restrict__ n_frames, int T, int F, int B,
                    double* __restrict__ rows, double* __restrict__ row_loss, float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int b = wv; b < B; b += FIN_WAVES) {
    const int len = row_count(n_frames, b, T);
    const int n = (int)chunks_of((long)len * F, CHUNK);            // <= nchunks
    const double* p = part + (long)b * nchunks;
    double a = 0.0;
    for (int k = lane; k < n; k += 64) a += p[k];
    a = wave_sum(a);
    const double r = len > 0 ? a / (double)len : 0.0;
    if (lane == 0) {
      rows[b] = r;
      if (row_loss) row_loss[b] = r;
    }
  }
  __syncthreads();                        // (the rows were written by this workgroup: visible to it behind the barrier)
  if (wv == 0) {
    double sum = 0.0;
    for (int b = lane; b < B; b += 64) sum += rows[b];
    sum = wave_sum(sum);
    if (lane == 0) loss[0] = (float)sum;
  }
}

inline long n_chunks(int T, int F) { return chunks_of((long)T * F, CHUNK); }
inline bool ok_shape(int B, int T, int F) {
  return B > 0 && B <= 65535 && T > 0 && F > 0 && (long)T * F <= (1L << 30) && n_chunks(T, F) * B < (1L << 31);
}
bool ok_spec(const Spec& s, int B) {
  return s.p && !((uintptr_t)s.p & 7) && s.st > 0 && s.sf > 0 && s.sb >= 0 && (B == 1 || s.sb > 0) && !((s.sb | s.st | s.sf) & 1);
}
// workspace: [partials B x nchunks doubles][rows B doubles], byte offsets
struct LossWs { size_t rows, total; };
inline LossWs loss_ws(int B, int T, int F) {
  LossWs w;
  w.rows = align_up((size_t)B * n_chunks(T, F) * sizeof(double), 256);
  w.total = w.rows + align_up((size_t)B * sizeof(double), 256);
  return w;
}

template <int KIND>
void launch_pass(int pred_mode, dim3 grid, hipStream_t s, const float* pred, const float* target, const Spec& X, const Spec& S,
                 const int* n_frames, int T, int F, double* part, float* dpred) {
  if (pred_mode == 1)
    hipLaunchKernelGGL((spectral_pass<KIND, 1>), grid, dim3(256), 0, s, pred, target, X, S, n_frames, T, F, part, dpred);
  else
    hipLaunchKernelGGL((spectral_pass<KIND, 2>), grid, dim3(256), 0, s, pred, target, X, S, n_frames, T, F, part, dpred);
}

}  // namespace

extern "C" size_t avvad_spectral_loss_workspace(int B, int T, int F) { return ok_shape(B, T, F) ? loss_ws(B, T, F).total : 0; }

extern "C" int avvad_spectral_loss(const float* pred, int pred_mode, int kind, const float* target, const float* mix, long mb,
                                   long mt, long mf, const float* speech, long sb, long st, long sf, const int* n_frames,
                                   float* loss, double* row_loss, float* dpred, int B, int T, int F, void* ws, size_t ws_bytes,
                                   avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!pred || !loss || !ws || kind < 0 || kind > 2 || pred_mode < 1 || pred_mode > 2 || !ok_shape(B, T, F)) return AVVAD_EINVAL;
  const Spec X = {mix, mb, mt, mf}, S = {speech, sb, st, sf};
  if ((kind < 2 && !target) || (kind >= 1 && !ok_spec(X, B)) || (kind == 2 && !ok_spec(S, B))) return AVVAD_EINVAL;
  if (ws_misaligned(ws) || ((uintptr_t)row_loss & 7)) return AVVAD_EINVAL;
  const LossWs w = loss_ws(B, T, F);
  if (ws_bytes < w.total) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  double* part = (double*)ws;
  double* rows = (double*)((char*)ws + w.rows);
  const int nchunks = (int)n_chunks(T, F);
  const dim3 grid((unsigned)nchunks, B);
  if (kind == 0) launch_pass<0>(pred_mode, grid, s, pred, target, X, S, n_frames, T, F, part, dpred);
  else if (kind == 1) launch_pass<1>(pred_mode, grid, s, pred, target, X, S, n_frames, T, F, part, dpred);
  else launch_pass<2>(pred_mode, grid, s, pred, target, X, S, n_frames, T, F, part, dpred);
  hipLaunchKernelGGL(spectral_finish, dim3(1), dim3(64 * FIN_WAVES), 0, s, part, nchunks, n_frames, T, F, B, rows, row_loss, loss);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
