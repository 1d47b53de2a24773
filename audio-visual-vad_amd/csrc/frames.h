// frames.h -- the framing + windowed-DFT operands shared by the STFT front-end (stft.hip) and the training labels
// (target.hip): a real DFT of every frame of a [B][L] batch is ONE fp32-MFMA GEMM, S[(b,t)][2f + {re,im}] =
// sum_k wave[b][t*hop + k] basis[k][2f + {re,im}], run through igemm::launch.
#pragma once
#include "igemm.h"

namespace frames {
namespace {     // internal linkage: every translation unit that includes this gets its own copy of the kernel

// A[m = (b,t)][k] = wave[b][t*hop + k]  (zero beyond the utterance: the reference's end padding)
struct FrameRows {
  static constexpr bool KCONTIG = true;
  static constexpr int VEC = 1;
  typedef igemm::NoCtx Ctx;
  const float* p;
  long L;
  int X, K, T, hop;
  __device__ __forceinline__ Ctx prep(int) const { return Ctx(); }
  __device__ __forceinline__ void load(const Ctx&, int x, int k0, int kin, float* v) const {
    const int k = k0 + kin;
    float t = 0.f;
    if (x < X && k < K) {
      const int b = x / T, fr = x - b * T;
      const long idx = (long)fr * hop + k;
      if (idx < L) t = p[(long)b * L + idx];
    }
    v[0] = t;
  }
};

// basis[k][2f] = hann[k] cos(2 pi f k / N), basis[k][2f+1] = -hann[k] sin(2 pi f k / N); columns >= 2F are zero
__global__ void dft_basis(float* __restrict__ W, int N, int F, int ld) {
  const long n = (long)N * ld;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int k = (int)(i / ld), c = (int)(i % ld);
    float v = 0.f;
    if (c < 2 * F) {
      const int f = c >> 1;
      const double win = 0.5 - 0.5 * cospi(2.0 * (double)k / (double)N);          // periodic Hann
      const long fk = ((long)f * k) % N;                                          // exact phase reduction
      const double ang = 2.0 * (double)fk / (double)N;
      v = (float)((c & 1) ? -win * sinpi(ang) : win * cospi(ang));
    }
    W[i] = v;
  }
}

static inline int grid1(long n) { long b = (n + 255) / 256; return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }
// row pitch (floats) of S: the 2F interleaved (re, im) columns rounded up to a float4
static inline int spectrum_ld(int n_fft) { return (2 * (n_fft / 2 + 1) + 3) / 4 * 4; }

// S [B*T][ld] = framed, windowed DFT of wave [B][L] (W: n_fft x ld basis scratch; slab: igemm::SLAB_FLOATS floats)
static inline int framed_dft(const float* wave, long L, int B, int T, int n_fft, int hop, float* W, float* S, float* slab,
                             hipStream_t s) {
  const int F = n_fft / 2 + 1, ld = spectrum_ld(n_fft);
  const int M = B * T;
  hipLaunchKernelGGL(dft_basis, dim3(grid1((long)n_fft * ld)), dim3(256), 0, s, W, n_fft, F, ld);
  FrameRows a{wave, L, M, n_fft, T, hop};
  igemm::ColPlain<4> b{W, ld, ld, n_fft, 0};
  igemm::EpiStore e{S, ld, nullptr, 0};
  return igemm::launch<128, 128>(a, b, e, M, ld, n_fft, 1, s, slab, /*allow_bf16=*/false);
}

}  // namespace
}  // namespace frames
