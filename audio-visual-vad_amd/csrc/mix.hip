// mix.hip -- clean speech and noise mixed at a target SNR on the GPU, for training: the mixture is made in the step from
// a clean batch and a noise bank instead of being read from a file that somebody mixed offline.
//
// Replaces: nothing the reference has -- its corpus module leaves the noise-aware dataset as a TODO
//   (packages/dataset/ntcd_timit.py:13, 246) and its training scripts read mixtures made offline at fixed SNRs.
//
// Row b: speech s = clean[b][0 .. len_b), noise n[i] = bank[clip_off[k] + (start[b] + i) mod clip_len[k]] (the clip read
// circularly), Es = sum s^2, En = sum n^2 over i < len_b (every value widened to double before it is squared),
//   g_b = (float) sqrt(Es / (En ratio[b]))       (double, rounded once; ratio = 10^(snr_db / 10) comes from the host)
//   noise_out[b][i] = g_b n[i]                   (one float product)
//   noisy[b][i]     = s[i] + noise_out[b][i]     (one float addition of that product: no contraction into an fma, so
//                                                 noisy - clean is the noise that was handed out, bit for bit)
// and exact zeros from len_b to L.  g_b = 0 when len_b <= 0, Es == 0, En == 0 or ratio[b] is not finite and positive.
//
// Kernel forms (memory-bound, and at a training batch's size launch-bound):
//   mix_energies: rows are cut into chunks of AVVAD_MIX_CHUNK samples; workgroup (chunk, row) has four waves whose 256
//        lanes stride over the chunk (plain dword loads: the row bases are only 4-byte aligned), cross-lane sums by a fixed
//        butterfly, the four waves added in wave order (reduce.h); the workgroup stores one (Es, En) partial.  A workgroup
//        whose chunk lies past the row's length exits and stores nothing.
//   mix_gain: one thread per row adds the row's partials in ascending chunk order (only the chunks below the row's length
//        are read), forms g_b, and zeroes peak[b].
//   mix_apply: the same grid over [0, L): the mixture, the scaled noise, the zeros behind the length; the workgroup's
//        max |noisy| (fmaxf from 0, as avvad_abs_max takes it) goes to peak[b] by an integer atomic maximum on its bit
//        pattern -- a maximum of non-negative floats has no order, so this equals avvad_abs_max of the written row.
//   The circular read: one 64-bit modulo per workgroup for the chunk's first sample; a clip of at least a chunk then
//        wraps at most once in the chunk and lanes wrap by compare-and-subtract; a shorter clip takes a 32-bit modulo
//        per sample (correct, slower).
// No floating-point atomics, and the chunking depends on the row length alone: bit-identical run to run, whatever the CU
// cap, and a row's outputs depend on that row alone.  Nothing of clean at or behind len_b is read.  Nothing outside
// [0, n_bank) is read whatever the device arrays hold: the clip index is clamped to [0, K), an offset outside the bank or
// a length below 1 makes the row's noise silent (nothing of the bank is read, g_b = 0), a clip that would run past n_bank
// is cut there, and start is taken mod the clip's length.
#include <math.h>

#include "reduce.h"

namespace {

constexpr int CHUNK = AVVAD_MIX_CHUNK;     // samples of one partial
constexpr int UN = 8;                      // samples in flight per lane in the energy pass (as scores.hip)
static_assert(CHUNK % (256 * UN) == 0, "a chunk is a whole number of unrolled workgroup strides");

// The row's clip as the kernels read it: `base` points at its first sample, `len` samples lie inside the bank (0: silent,
// nothing is read), `pos` is the clip position of row sample i0.  Uniform for the workgroup.
struct Clip { const float* base; int len; int pos; };
__device__ __forceinline__ Clip row_clip(const float* __restrict__ bank, long n_bank, const long long* __restrict__ clip_off,
                                         const int* __restrict__ clip_len, int K, const int* __restrict__ clip,
                                         const int* __restrict__ start, int b, long i0) {
  int k = clip[b];
  k = k < 0 ? 0 : (k >= K ? K - 1 : k);
  const long long off = clip_off[k];
  long cl = clip_len[k];
  Clip c = {bank, 0, 0};
  if (off < 0 || off >= n_bank || cl < 1) return c;
  if (cl > n_bank - off) cl = n_bank - off;
  long st = (long)start[b] % cl;
  if (st < 0) st += cl;
  c.base = bank + off;
  c.len = (int)cl;
  c.pos = (int)((st + i0) % cl);
  return c;
}
// clip position of the sample d (< CHUNK) behind the chunk's first
__device__ __forceinline__ int clip_at(const Clip& c, int d) {
  const unsigned p = (unsigned)c.pos + (unsigned)d;       // pos < len < 2^31, d < CHUNK: no overflow
  if (c.len >= CHUNK) return (int)(p >= (unsigned)c.len ? p - (unsigned)c.len : p);   // d < CHUNK <= len: wraps at most once
  return (int)(p % (unsigned)c.len);
}

// part[row][chunk][2] = (Es, En) of the chunk, chunk < nchunks(L)
__global__ void __launch_bounds__(256)
    mix_energies(const float* __restrict__ clean, long ld_clean, const int* __restrict__ n_samples, const float* __restrict__ bank,
                 long n_bank, const long long* __restrict__ clip_off, const int* __restrict__ clip_len, int K,
                 const int* __restrict__ clip, const int* __restrict__ start, long L, double* __restrict__ part) {
  __shared__ double red[2][4];
  const int b = blockIdx.y;
  const long len = row_len(n_samples, b, L);
  const long i0 = (long)blockIdx.x * CHUNK;
  if (i0 >= len) return;                  // (uniform for the workgroup: nothing is waiting at the barrier below)
  const int n = (int)min((long)CHUNK, len - i0);
  const float* s = clean + b * ld_clean + i0;
  const Clip c = row_clip(bank, n_bank, clip_off, clip_len, K, clip, start, b, i0);
  double es = 0.0, en = 0.0;
  for (int d0 = threadIdx.x; d0 < n; d0 += 256 * UN) {
    float vs[UN] = {}, vn[UN] = {};
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int d = d0 + u * 256;
      if (d < n) {
        vs[u] = s[d];
        if (c.len) vn[u] = c.base[clip_at(c, d)];
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {         // (a lane past the end adds exact zeros)
      const double ds = (double)vs[u], dn = (double)vn[u];
      es += ds * ds;
      en += dn * dn;
    }
  }
  const double e[2] = {es, en};
  fold4_put(red, e, Add());
  __syncthreads();
  if (threadIdx.x < 2) {
    const int q = threadIdx.x;
    part[((long)b * gridDim.x + blockIdx.x) * 2 + q] = fold4_get(red[q], Add());
  }
}

// one thread per row: the partials in ascending chunk order -> g_b; peak[b] = 0 for mix_apply's maxima
__global__ void __launch_bounds__(64)
    mix_gain(const double* __restrict__ part, int nchunks, const int* __restrict__ n_samples, long L, const double* __restrict__ ratio,
             int B, float* __restrict__ g_ws, float* __restrict__ gain, double* __restrict__ energies, float* __restrict__ peak) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long len = row_len(n_samples, b, L);
  const int n = (int)chunks_of(len, CHUNK);            // <= nchunks
  const double* p = part + (long)b * nchunks * 2;
  double es = 0.0, en = 0.0;
  for (int k = 0; k < n; ++k) es += p[2 * k], en += p[2 * k + 1];
  const double r = ratio[b];
  float g = 0.f;
  if (len > 0 && es != 0.0 && en != 0.0 && r > 0.0 && r < (double)INFINITY) g = (float)sqrt(es / (en * r));
  g_ws[b] = g;
  if (gain) gain[b] = g;
  if (energies) energies[2 * b] = es, energies[2 * b + 1] = en;
  if (peak) peak[b] = 0.f;
}

// noisy / noise_out over [0, L) of the row, and the workgroup's max |noisy| into peak[b]
__global__ void __launch_bounds__(256)
    mix_apply(const float* __restrict__ clean, long ld_clean, const int* __restrict__ n_samples, const float* __restrict__ bank,
              long n_bank, const long long* __restrict__ clip_off, const int* __restrict__ clip_len, int K,
              const int* __restrict__ clip, const int* __restrict__ start, const float* __restrict__ g_ws, long L,
              float* __restrict__ noisy, long ld_noisy, float* __restrict__ noise_out, long ld_noise, float* __restrict__ peak) {
  __shared__ float red[4];
  const int b = blockIdx.y;
  const long len = row_len(n_samples, b, L);
  const long i0 = (long)blockIdx.x * CHUNK;
  const int n = (int)min((long)CHUNK, L - i0);                           // columns of this chunk (> 0: the grid covers L)
  const int nv = len > i0 ? (int)min((long)CHUNK, len - i0) : 0;         // ... of which below the row's length
  const float g = g_ws[b];
  const float* s = clean + b * ld_clean + i0;
  float* y = noisy + b * ld_noisy + i0;
  float* z = noise_out ? noise_out + b * ld_noise + i0 : nullptr;
  Clip c = {bank, 0, 0};
  if (nv > 0 && g != 0.f) c = row_clip(bank, n_bank, clip_off, clip_len, K, clip, start, b, i0);
  float m = 0.f;
#pragma unroll 4
  for (int d = threadIdx.x; d < n; d += 256) {
    float v = 0.f, gn = 0.f;
    if (d < nv) {
      v = s[d];
      if (c.len) {                        // (g == 0 leaves the speech as it is, a -0 included)
#pragma clang fp contract(off)            // a rounded product, then a rounded sum: hipcc would fuse them (-ffp-contract=fast)
        gn = g * c.base[clip_at(c, d)];
        v = v + gn;
      }
    }
    y[d] = v;
    if (z) z[d] = gn;
    m = fmaxf(m, fabsf(v));
  }
  if (!peak) return;                      // (uniform)
  fold4_put(red, m, fmaxf);
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fold4_get(red, fmaxf);
    // m >= 0 and not a NaN (fmaxf from 0 drops NaN, as avvad_abs_max does): its bits order like the value
    if (m > 0.f) atomicMax((unsigned int*)peak + b, __builtin_bit_cast(unsigned int, m));
  }
}

inline long n_chunks(long L) { return chunks_of(L, CHUNK); }
inline bool ok_shape(int B, long L) {
  return B > 0 && B <= 65535 && L > 0 && L < (1L << 40) && n_chunks(L) * B < (1L << 31) / 2;
}
// workspace: [partials B x nchunks x 2 doubles][g B floats], byte offsets
struct MixWs { size_t g, total; };
inline MixWs mix_ws(int B, long L) {
  MixWs w;
  w.g = align_up((size_t)B * n_chunks(L) * 2 * sizeof(double), 256);
  w.total = w.g + align_up((size_t)B * sizeof(float), 256);
  return w;
}

}  // namespace

extern "C" size_t avvad_mix_workspace(int B, long L) { return ok_shape(B, L) ? mix_ws(B, L).total : 0; }

extern "C" int avvad_mix(const float* clean, long ld_clean, const int* n_samples, const float* bank, long n_bank,
                         const long long* clip_off, const int* clip_len, int K, const int* clip, const int* start,
                         const double* ratio, float* noisy, long ld_noisy, float* noise_out, long ld_noise, float* gain,
                         double* energies, float* peak, int B, long L, void* ws, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!clean || !bank || !clip_off || !clip_len || !clip || !start || !ratio || !noisy || !ws) return AVVAD_EINVAL;
  if (!ok_shape(B, L) || K < 1 || n_bank < 1 || ld_clean < L || ld_noisy < L || (noise_out && ld_noise < L)) return AVVAD_EINVAL;
  if (noisy == clean || (noise_out && (noise_out == clean || noise_out == noisy))) return AVVAD_EINVAL;
  if (ws_misaligned(ws) || ((uintptr_t)ratio & 7) || ((uintptr_t)energies & 7) || ((uintptr_t)clip_off & 7)) return AVVAD_EINVAL;
  const MixWs w = mix_ws(B, L);
  if (ws_bytes < w.total) return AVVAD_EWORKSPACE;
  hipStream_t s = (hipStream_t)sv;
  double* part = (double*)ws;
  float* g_ws = (float*)((char*)ws + w.g);
  const dim3 grid((unsigned)n_chunks(L), B);
  hipLaunchKernelGGL(mix_energies, grid, dim3(256), 0, s, clean, ld_clean, n_samples, bank, n_bank, clip_off, clip_len, K, clip,
                     start, L, part);
  hipLaunchKernelGGL(mix_gain, dim3((B + 63) / 64), dim3(64), 0, s, part, (int)n_chunks(L), n_samples, L, ratio, B, g_ws, gain,
                     energies, peak);
  hipLaunchKernelGGL(mix_apply, grid, dim3(256), 0, s, clean, ld_clean, n_samples, bank, n_bank, clip_off, clip_len, K, clip, start,
                     g_ws, L, noisy, ld_noisy, noise_out, ld_noise, peak);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
