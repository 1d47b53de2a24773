// score_lab.hip -- which load form should the energy-ratio pass (csrc/scores.hip, gram_partials) use?  A stand-alone
// program: the pass over estimate, clean and mixture (12 bytes per sample, six double products per sample, one 6-double
// partial per 4096-sample chunk), in three load forms, timed with device events at the sizes of tools/mb_score.py.
//   form 0  plain dword loads, the workgroup's 256 lanes striding over the chunk (256 consecutive bytes per wave and
//           load), UN samples of each signal in flight per lane: works for any 4-byte aligned row (the production form)
//   form 1  dwordx4 loads, a lane takes four consecutive samples (1 KB per wave and load), UN/4 loads of each signal
//           in flight: needs all three rows 16-byte aligned (contiguous tensors whose length is a multiple of 4)
//   form 2  the lane-to-sample assignment of form 1 read with dword loads (lane stride 16 bytes): what rows that are
//           not 16-byte aligned would need if both forms had to give the same bits
// "warm": the same buffers every launch (L2 / Infinity Cache resident below 256 MB); "cold": launches rotate over copies
// with a footprint above 600 MB.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/lab/score_lab.hip -o score_lab && ./score_lab
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#define CK(x)                                                                         \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) {                                                           \
      fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);     \
      exit(1);                                                                        \
    }                                                                                 \
  } while (0)

constexpr int CHUNK = 4096;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void add6(double* g, float e, float r, float x) {
  const double de = (double)e, dr = (double)r, dn = (double)x - dr;
  g[0] += de * de, g[1] += de * dr, g[2] += de * dn, g[3] += dr * dr, g[4] += dn * dn, g[5] += dr * dn;
}

template <int FORM, int UN>
__global__ void __launch_bounds__(256)
    partials(const float* __restrict__ est, const float* __restrict__ ref, const float* __restrict__ mix, long L, double* __restrict__ part) {
  __shared__ double red[6][4];
  const int b = blockIdx.y;
  const long i0 = (long)blockIdx.x * CHUNK, i1 = min(L, i0 + CHUNK);
  const float *e = est + b * L, *r = ref + b * L, *x = mix + b * L;
  double g[6] = {};
  if (FORM == 0) {
    for (long i = i0 + threadIdx.x; i < i1; i += 256 * UN) {
      float ve[UN] = {}, vr[UN] = {}, vx[UN] = {};
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const long j = i + u * 256;
        if (j < i1) ve[u] = e[j], vr[u] = r[j], vx[u] = x[j];
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) add6(g, ve[u], vr[u], vx[u]);
    }
  } else {
    constexpr int U4 = UN / 4 > 0 ? UN / 4 : 1;
    for (long i = i0 + 4 * threadIdx.x; i < i1; i += 1024 * U4) {
      float4 ve[U4] = {}, vr[U4] = {}, vx[U4] = {};
#pragma unroll
      for (int u = 0; u < U4; ++u) {
        const long j = i + u * 1024;
        if (FORM == 1) {
          if (j + 3 < i1) {
            ve[u] = *reinterpret_cast<const float4*>(e + j);
            vr[u] = *reinterpret_cast<const float4*>(r + j);
            vx[u] = *reinterpret_cast<const float4*>(x + j);
          } else {
            float *pe = &ve[u].x, *pr = &vr[u].x, *px = &vx[u].x;
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (j + k < i1) pe[k] = e[j + k], pr[k] = r[j + k], px[k] = x[j + k];
          }
        } else {
          float *pe = &ve[u].x, *pr = &vr[u].x, *px = &vx[u].x;
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (j + k < i1) pe[k] = e[j + k], pr[k] = r[j + k], px[k] = x[j + k];
        }
      }
#pragma unroll
      for (int u = 0; u < U4; ++u) {
        add6(g, ve[u].x, vr[u].x, vx[u].x);
        add6(g, ve[u].y, vr[u].y, vx[u].y);
        add6(g, ve[u].z, vr[u].z, vx[u].z);
        add6(g, ve[u].w, vr[u].w, vx[u].w);
      }
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const double s = wave_sum_d(g[c]);
    if (lane == 0) red[c][wv] = s;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int c = threadIdx.x;
    part[((long)b * gridDim.x + blockIdx.x) * 6 + c] = ((red[c][0] + red[c][1]) + red[c][2]) + red[c][3];
  }
}

typedef void (*Kernel)(const float*, const float*, const float*, long, double*);
struct Form {
  const char* name;
  Kernel k;
};

int main() {
  const Form forms[] = {{"dword  un4", partials<0, 4>}, {"dword  un8", partials<0, 8>}, {"dwordx4 un4", partials<1, 4>},
                        {"dwordx4 un8", partials<1, 8>}, {"dword lane-stride-16B un4", partials<2, 4>}};
  const int nforms = sizeof(forms) / sizeof(forms[0]);
  const long shapes[][2] = {{1, 80000}, {16, 80000}, {64, 160000}};
  const int iters = 200, windows = 3;
  for (auto& sh : shapes) {
    const int B = (int)sh[0];
    const long L = sh[1], n = B * L;
    const long nch = (L + CHUNK - 1) / CHUNK;
    const long sets = std::max(1L, std::min(640L, (long)(600e6 / (12.0 * n)) + 1));
    float* buf;
    double* part;
    CK(hipMalloc(&buf, sizeof(float) * 3 * n * sets));
    CK(hipMalloc(&part, sizeof(double) * 6 * B * nch));
    std::vector<float> h(3 * n);
    unsigned s = 12345u + (unsigned)n;
    for (auto& v : h) s = s * 1664525u + 1013904223u, v = ((int)(s >> 8) % 20001 - 10000) * 1e-4f;
    for (long k = 0; k < sets; ++k) CK(hipMemcpy(buf + 3 * n * k, h.data(), sizeof(float) * 3 * n, hipMemcpyHostToDevice));
    std::vector<double> ref(6 * B * nch), got(6 * B * nch);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int cold = 0; cold < 2; ++cold) {
      std::vector<std::vector<float>> us(nforms);
      for (int w = 0; w < windows + 1; ++w)               // window 0 is the warm-up of every form
        for (int f = 0; f < nforms; ++f) {
          CK(hipEventRecord(e0, 0));
          for (int it = 0; it < iters; ++it) {
            const float* p = buf + 3 * n * (cold ? it % sets : 0);
            hipLaunchKernelGGL(forms[f].k, dim3((unsigned)nch, B), dim3(256), 0, 0, p, p + n, p + 2 * n, L, part);
          }
          CK(hipEventRecord(e1, 0));
          CK(hipEventSynchronize(e1));
          CK(hipGetLastError());
          float ms;
          CK(hipEventElapsedTime(&ms, e0, e1));
          if (w) us[f].push_back(ms * 1e3f / iters);
          else {
            CK(hipMemcpy(got.data(), part, sizeof(double) * got.size(), hipMemcpyDeviceToHost));
            if (f == 0) ref = got;
            double worst = 0;
            for (size_t i = 0; i < got.size(); ++i) worst = std::max(worst, std::abs(got[i] - ref[i]) / (std::abs(ref[i]) + 1e-300));
            if (worst > 1e-9) {
              fprintf(stderr, "form %s differs from form 0: %g relative\n", forms[f].name, worst);
              return 1;
            }
          }
        }
      for (int f = 0; f < nforms; ++f) {
        const float best = *std::min_element(us[f].begin(), us[f].end());
        printf("B %3d L %6ld %s %-26s us/launch", B, L, cold ? "cold" : "warm", forms[f].name);
        for (float v : us[f]) printf(" %8.2f", v);
        printf("   best: %6.3f TB/s of the 12 bytes per sample\n", 12.0 * n / (best * 1e-6) / 1e12);
      }
    }
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    CK(hipFree(buf));
    CK(hipFree(part));
  }
  return 0;
}
