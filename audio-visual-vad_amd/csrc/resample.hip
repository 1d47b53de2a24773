// resample.hip -- rational-rate resampling of waveforms, whole utterances and streams: what stands between audio of any
// rate and the 16 kHz signal chain.  The filter is scipy.signal.resample_poly's default (a Kaiser-windowed sinc of
// 2 half + 1 taps, half = 10 max(up, down), built on the host in float64); the definition, per row of L inputs x:
//   out[n] = sum_m h[n down + half - m up] x[m],   m ascending over max(0, ceil((n down - half) / up)) ..
//            min(L - 1, floor((n down + half) / up)),   0 <= n < ceil(L up / down)
// Inputs that do not exist are skipped, not multiplied.  Every product and the whole chain are double fma, the sum is
// rounded to float once; so a value depends on its own inputs alone -- not on the tile, the row, the batch, "max_cus", the
// LDS / global choice below or how a stream was cut into calls.
//
// TAPS.  The caller hands the taps PHASE-MAJOR: with T = 2 half / up + 1, taps[p T + j] = h[p + j up] (0 where that lies
// behind the last tap, never read).  Output n with q = n down + half has phase p = q mod up and newest input mq = q / up;
// input m meets taps[p T + (mq - m)]: one output's taps are contiguous.
//
// SHAPE.  One workgroup per (row, tile of AVVAD_RESAMPLE_TILE outputs), one output per thread.  The tile's input span
// (about TILE down / up + T samples) is staged once in LDS through coalesced dword loads -- any 4-byte aligned row -- and
// the taps table too when it has at most RS_TAPS_LDS doubles; a larger table (160/441: 8 960, 800/999: 20 000) is read from
// global memory, where it stays in L2, and a span beyond RS_X_LDS floats (decimation by more than about 29) is read from
// global memory as well.  The arithmetic is one text (rs_tile) for the four forms.
//
// STREAM.  The same body fed from state ++ chunk: row b has taken in_before[b] inputs and emitted out_before[b] outputs
// (host clock, 64-bit: n down passes 2^31 within hours), takes n_valid[b] more and emits n_emit[b].  state [B][H],
// H = 2 half / up + 2, holds the last H inputs; an output that has not been emitted needs at most H - 2 of them.
#include <numeric>

#include "reduce.h"

namespace {

constexpr int RS_NT = AVVAD_RESAMPLE_TILE;      // threads of a workgroup = outputs of a tile
constexpr int RS_TAPS_LDS = 4096;               // doubles of taps a workgroup stages (32 KB)
constexpr int RS_X_LDS = 7680;                  // floats of input span a workgroup stages (30 KB): 62 KB with the taps
constexpr long long RS_POS_MAX = 1LL << 50;     // absolute positions are clamped here: n down + half stays within 64 bits

struct RsRatio {
  int up, down, half, T, H;
  long n_taps;                                  // up T
};
bool rs_ratio(int up, int down, RsRatio* r) {
  if (up < 1 || down < 1 || up > AVVAD_RESAMPLE_MAX_RATE || down > AVVAD_RESAMPLE_MAX_RATE || std::gcd(up, down) != 1 ||
      (up == 1 && down == 1))
    return false;
  r->up = up;
  r->down = down;
  r->half = 10 * (up > down ? up : down);
  r->T = 2 * r->half / up + 1;
  r->H = r->T + 1;
  r->n_taps = (long)up * r->T;
  return true;
}
// the most inputs a tile's outputs span (first output's oldest tap to last output's newest input)
long rs_span(const RsRatio& r) { return (long)(RS_NT - 1) * r.down / r.up + r.T + 2; }

// Where a row's inputs lie: absolute input m is a[m - a0] for m < b0 and b[m - b0] from b0 on; [lo, hi] are the inputs that
// exist.  A whole utterance is one piece (a0 = b0 = lo = 0); a stream is its state and the call's chunk.
struct RsSrc {
  const float *a, *b;
  long long a0, b0, lo, hi;
  __device__ __forceinline__ float at(long long m) const { return m < b0 ? a[m - a0] : b[m - b0]; }
};

// A tile: `cells` (<= RS_NT) cells of out from the row's absolute output n0 on, of which the first cnt are computed and the
// rest are +0.  Uniform per workgroup: every thread reaches the barrier.
template <bool TL, bool XL>
__device__ __forceinline__ void rs_tile(const RsSrc& s, const double* __restrict__ taps, int up, int down, int half, int T,
                                        long long n0, int cnt, int cells, float* __restrict__ out, double* lt, float* xs) {
  const int tid = threadIdx.x;
  const long long q0 = n0 * down + half, mq0 = q0 / up;
  const int p0 = (int)(q0 - mq0 * up);
  const long long mb = mq0 - (T - 1);                     // the first output's oldest possible input
  if (TL) {
    for (int i = tid; i < up * T; i += RS_NT) lt[i] = taps[i];
  }
  if (XL && cnt > 0) {
    const int span = (int)((p0 + (long long)(cnt - 1) * down) / up) + T;     // .. the last output's newest input
    for (int i = tid; i < span; i += RS_NT) {
      const long long m = mb + i;
      xs[i] = (m >= s.lo && m <= s.hi) ? s.at(m) : 0.f;
    }
  }
  if (TL || XL) __syncthreads();
  if (tid >= cells) return;
  float y = 0.f;
  if (tid < cnt) {
    const int r = p0 + tid * down;                        // < 2^31: 255 * 1024 + 1024
    const long long mq = mq0 + r / up;
    const int p = r % up;
    const long long oldest = mq - (2 * half - p) / up;
    const long long m0 = oldest > s.lo ? oldest : s.lo, m1 = mq < s.hi ? mq : s.hi;
    const double* tp = (TL ? lt : taps) + (long)p * T;
    double acc = 0.0;
    for (long long m = m0; m <= m1; ++m) acc = fma(tp[(int)(mq - m)], (double)(XL ? xs[(int)(m - mb)] : s.at(m)), acc);
    y = (float)acc;
  }
  out[tid] = y;
}

struct RsLds {
  double* lt;
  float* xs;
};
template <bool TL>
__device__ __forceinline__ RsLds rs_carve(double* lds, int up, int T) {
  return {lds, reinterpret_cast<float*>(lds + (TL ? up * T : 0))};
}

template <bool TL, bool XL>
__global__ void __launch_bounds__(RS_NT)
    rs_whole_kernel(const float* __restrict__ x, long ld_x, const int* __restrict__ lengths, const double* __restrict__ taps, int up,
                    int down, int half, int T, float* __restrict__ out, long ld_out, int* __restrict__ n_out, long L, long Lout) {
  extern __shared__ __attribute__((aligned(16))) double rs_lds[];
  const RsLds l = rs_carve<TL>(rs_lds, up, T);
  const int b = blockIdx.y;
  const long len = row_len(lengths, b, L);
  const long no = (len * up + down - 1) / down;
  if (n_out && blockIdx.x == 0 && threadIdx.x == 0) n_out[b] = (int)no;
  const long n0 = (long)blockIdx.x * RS_NT;
  const long left = Lout - n0, have = no - n0;
  const int cells = left < RS_NT ? (int)left : RS_NT;
  const int cnt = have < 0 ? 0 : (have < cells ? (int)have : cells);
  const float* row = x + (long)b * ld_x;
  const RsSrc s{row, row, 0, 0, 0, len - 1};
  rs_tile<TL, XL>(s, taps, up, down, half, T, n0, cnt, cells, out + (long)b * ld_out + n0, l.lt, l.xs);
}

__device__ __forceinline__ long long rs_clamp(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Every count is clamped, so that wrong ones cannot reach outside a buffer.
template <bool TL, bool XL>
__global__ void __launch_bounds__(RS_NT)
    rs_stream_kernel(const float* __restrict__ chunk, long ld_chunk, const long long* __restrict__ n_valid,
                     const long long* __restrict__ in_before, const long long* __restrict__ out_before,
                     const long long* __restrict__ n_emit, const float* __restrict__ state_in, float* __restrict__ state_out,
                     const double* __restrict__ taps, int up, int down, int half, int T, int H, float* __restrict__ out, long ld_out,
                     int n_in, int n_max) {
  extern __shared__ __attribute__((aligned(16))) double rs_lds[];
  const RsLds l = rs_carve<TL>(rs_lds, up, T);
  const int b = blockIdx.y;
  const long long nv = rs_clamp(n_valid[b], n_in), ib = rs_clamp(in_before[b], RS_POS_MAX), ob = rs_clamp(out_before[b], RS_POS_MAX);
  const int ne = (int)rs_clamp(n_emit[b], n_max);
  const RsSrc s{state_in + (long)b * H, chunk + (long)b * ld_chunk, ib - H, ib, ib > H ? ib - H : 0, ib + nv - 1};
  const long t0 = (long)blockIdx.x * RS_NT;
  const long left = n_max - t0, have = ne - t0;
  const int cells = left < 0 ? 0 : (left < RS_NT ? (int)left : RS_NT);
  const int cnt = have < 0 ? 0 : (have < cells ? (int)have : cells);
  rs_tile<TL, XL>(s, taps, up, down, half, T, ob + t0, cnt, cells, out + (long)b * ld_out + t0, l.lt, l.xs);
  if (blockIdx.x == 0) {                                    // the new state: the last H of state ++ chunk[:nv]
    for (int k = threadIdx.x; k < H; k += RS_NT) state_out[(long)b * H + k] = s.at(ib + nv - H + k);
  }
}

// which of the four forms a ratio takes, and their dynamic LDS
struct RsPlan {
  bool tl, xl;
  size_t lds;
};
RsPlan rs_plan(const RsRatio& r) {
  RsPlan p;
  p.tl = r.n_taps <= RS_TAPS_LDS;
  p.xl = rs_span(r) <= RS_X_LDS;
  p.lds = (p.tl ? (size_t)r.n_taps * sizeof(double) : 0) + (p.xl ? (size_t)rs_span(r) * sizeof(float) : 0);
  return p;
}

}  // namespace

extern "C" long avvad_resample_length(long L, int up, int down) {
  RsRatio r;
  if (L < 0 || !rs_ratio(up, down, &r) || L > (1L << 40)) return 0;
  return (L * up + down - 1) / down;
}
extern "C" long avvad_resample_taps_len(int up, int down) {
  RsRatio r;
  return rs_ratio(up, down, &r) ? r.n_taps : 0;
}
extern "C" int avvad_resample_hist(int up, int down) {
  RsRatio r;
  return rs_ratio(up, down, &r) ? r.H : 0;
}

extern "C" int avvad_resample(const float* x, long ld_x, const int* lengths, const double* taps, int up, int down, float* out,
                              long ld_out, int* n_out, int B, long L, avvad_stream_t sv) {
  AVVAD_ENTER();
  RsRatio r;
  if (!rs_ratio(up, down, &r) || B < 1 || B > 65535 || L < 1 || L > 0x7fffffffL || !x || !taps || !out || ld_x < L) return AVVAD_EINVAL;
  const long Lout = avvad_resample_length(L, up, down);
  if (Lout > 0x7fffffffL || ld_out < Lout || ((uintptr_t)taps & 7)) return AVVAD_EINVAL;
  const RsPlan p = rs_plan(r);
  const dim3 grid(cdiv(Lout, RS_NT), B);
  const auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(RS_NT), p.lds, (hipStream_t)sv, x, ld_x, lengths, taps, up, down, r.half, r.T, out, ld_out,
                       n_out, L, Lout);
  };
  if (p.tl) p.xl ? go(rs_whole_kernel<true, true>) : go(rs_whole_kernel<true, false>);
  else p.xl ? go(rs_whole_kernel<false, true>) : go(rs_whole_kernel<false, false>);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

extern "C" int avvad_resample_stream(const float* chunk, long ld_chunk, const long long* n_valid, const long long* in_before,
                                     const long long* out_before, const long long* n_emit, const float* state_in, float* state_out,
                                     const double* taps, int up, int down, float* out, long ld_out, int B, int n_in, int n_max,
                                     avvad_stream_t sv) {
  AVVAD_ENTER();
  RsRatio r;
  if (!rs_ratio(up, down, &r) || B < 1 || B > 65535 || n_in < 0 || n_max < 0 || !n_valid || !in_before || !out_before || !n_emit ||
      !state_in || !state_out || state_in == state_out || !taps || ((uintptr_t)taps & 7) || (n_in > 0 && (!chunk || ld_chunk < n_in)) ||
      (n_max > 0 && (!out || ld_out < n_max)))
    return AVVAD_EINVAL;
  const RsPlan p = rs_plan(r);
  const dim3 grid(n_max > 0 ? cdiv(n_max, RS_NT) : 1, B);
  const auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(RS_NT), p.lds, (hipStream_t)sv, chunk, ld_chunk, n_valid, in_before, out_before, n_emit,
                       state_in, state_out, taps, up, down, r.half, r.T, r.H, out, ld_out, n_in, n_max);
  };
  if (p.tl) p.xl ? go(rs_stream_kernel<true, true>) : go(rs_stream_kernel<true, false>);
  else p.xl ? go(rs_stream_kernel<false, true>) : go(rs_stream_kernel<false, false>);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
