// trunk.hip -- ResNet-18 trunk over gray lip crops: forward and backward.
//
// Replaces `self.features(video).squeeze()` (+ the 3x channel repeat in front of it)
// of the reference: packages/models/Video_Net.py:60-81, packages/models/AV_Net.py:78-94,
// i.e. torchvision.models.resnet18 children [:-1].
//
// Data layout in HBM: activations NHWC fp32 (channel-contiguous: an im2col row
// is a run of 128-byte lines), weights re-packed once per call from the
// state_dict's OIHW into [(kh,kw,c)][co] (forward B operand) and
// [(kh,kw,co)][c] (dgrad B operand).  The reference's 3 identical input
// channels are folded into the stem's weights (sum over c), so the frame is
// read once as a 1-channel image.
//
// Kernels: every convolution (forward, dgrad, wgrad) is the fp32-MFMA
// implicit GEMM of igemm.h; BatchNorm statistics are a two-stage column
// reduction in fp64; normalisation / ReLU / residual add / pooling are fused
// elementwise kernels with 16-byte accesses.
#include "bgemm.h"
#include "conv64.h"

using convop::Geom;

namespace {

#include "bn_kernels.h"

constexpr int NCONV = AVVAD_TRUNK_NCONV;

// ------------------------------------------------------------------ static network description
constexpr int NBLOCK = 8;                             // 4 stages x 2 residual blocks
constexpr int WIDTHS[4] = {64, 128, 256, 512};        // channels of a stage

// One residual block: out = relu(bn2(conv2(a1)) + identity), a1 = relu(bn1(conv1(in))); identity = in, or with `ds` (the
// first block of stages 1..3) bnd(convd(in)).  Tensor offsets are in floats of the workspace; NHWC, M x width each.
struct Block {
  int stage, width;
  int h, w;          // output grid (of all its convolutions)
  long M;            // N * h * w: rows of its tensors
  bool ds;           // stride-2 entry, downsample convolution on the identity branch
  int i1, i2, id;    // its convolutions in the order of include/avvad.h (id: -1 without ds)
  size_t in;         // the block's input: the pooled stem output or the previous block's `out`
  size_t c1, a1;     // conv1's raw output; relu(bn1(c1))
  size_t c2, cd;     // conv2's raw output; the downsample convolution's (ds only)
  size_t out, qm;    // the block's output; its ReLU mask, one BYTE per quad of `out` (save_for_backward)
};

struct Plan {
  int h[6], w[6];  // 0: input, 1: stem out, 2: pooled / stage0, 3..5: stage1..3
  Geom geom[NCONV];                  // the convolutions in the order of include/avvad.h
  Block block[NBLOCK];
  // workspace offsets in floats
  size_t wf[NCONV], wd[NCONV];
  size_t wf16[NCONV], wd16[NCONV];   // bf16 packs of the bf16 data path: [co][(cc,tap,r)] and [c][(cc,tap,r)] (64-channel chunks cc)
  size_t bn_scale, bn_shift, bn_mean, bn_invstd;  // [NCONV][MAXC]
  size_t coef;                                    // [3][MAXC] backward coefficients
  size_t part;                                    // doubles: [STAT_CHUNKS][2][MAXC]
  size_t c0, p0, am;   // am: arg-max position (0..8, one byte per channel) of every pooled stem element
  size_t G[4], g0, wg[NCONV];   // wg[i]: conv i's packed weight gradient (all 20 kept: ONE unpack launch at the end)
  size_t slab;     // igemm::SLAB_FLOATS: partial tiles of the engine's stream-K round
  size_t total;
};

static bool trunk_desc_ok(const avvad_trunk_desc* d) { return d && d->N > 0 && d->H >= 32 && d->W >= 32; }
static Plan make_plan(const avvad_trunk_desc* d) {
  Plan p;
  p.h[0] = d->H; p.w[0] = d->W;
  // every halving -- 7x7 / 2 pad 3, the 3x3 / 2 pad 1 pool and stage entries -- is (n + 2 pad - ks) / 2 + 1 = (n - 1) / 2 + 1
  for (int s = 1; s < 6; ++s) { p.h[s] = (p.h[s - 1] - 1) / 2 + 1; p.w[s] = (p.w[s - 1] - 1) / 2 + 1; }
  // the network, once: the stem, then 4 stages x 2 blocks, a stride-2 entry with a downsample in the first block of stages 1..3
  int i = 0;
  auto add_conv = [&](int cin, int cout, int ks, int stride, int pad, int hin, int win, int ho, int wo) {
    p.geom[i] = {d->N, hin, win, cin, ho, wo, cout, ks, stride, pad};
    return i++;
  };
  add_conv(1, 64, 7, 2, 3, p.h[0], p.w[0], p.h[1], p.w[1]);
  int cin = 64;
  for (int s = 0; s < 4; ++s)
    for (int b = 0; b < 2; ++b) {
      Block& k = p.block[s * 2 + b];
      k.stage = s; k.width = WIDTHS[s]; k.ds = b == 0 && s > 0;
      k.h = p.h[s + 2]; k.w = p.w[s + 2]; k.M = (long)d->N * k.h * k.w;
      const int hin = k.ds ? p.h[s + 1] : k.h, win = k.ds ? p.w[s + 1] : k.w;
      k.i1 = add_conv(cin, k.width, 3, k.ds ? 2 : 1, 1, hin, win, k.h, k.w);
      k.i2 = add_conv(k.width, k.width, 3, 1, 1, k.h, k.w, k.h, k.w);
      k.id = k.ds ? add_conv(cin, k.width, 1, 2, 0, hin, win, k.h, k.w) : -1;
      cin = k.width;
    }
  // the workspace (the order and sizes of the parts are the layout avvad_trunk_workspace / avvad_trunk_activation publish)
  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += align_up(n, 64); return o; };
  auto weights = [&](int j) { const Geom& g = p.geom[j]; return (size_t)g.KS * g.KS * g.C * g.Co; };
  for (i = 0; i < NCONV; ++i) {
    const size_t n = weights(i);
    p.wf[i] = take(n);
    p.wd[i] = (i == 0) ? 0 : take(n);
    p.wf16[i] = (i == 0) ? 0 : take(n / 2);
    p.wd16[i] = (i == 0) ? 0 : take(n / 2);
  }
  p.bn_scale = take(NCONV * MAXC); p.bn_shift = take(NCONV * MAXC);
  p.bn_mean = take(NCONV * MAXC); p.bn_invstd = take(NCONV * MAXC);
  p.coef = take(3 * MAXC);
  p.part = take((size_t)STAT_CHUNKS * 2 * MAXC * 2);  // doubles
  p.slab = take(igemm::SLAB_FLOATS);
  const size_t N = d->N;
  p.c0 = take(N * p.h[1] * p.w[1] * 64);
  p.p0 = take(N * p.h[2] * p.w[2] * 64);
  p.am = take(N * p.h[2] * p.w[2] * 16);     // 4 bytes (one channel quad) per word
  size_t in = p.p0;
  for (Block& k : p.block) {
    const size_t n = (size_t)k.M * k.width;
    k.in = in;
    k.c1 = take(n); k.a1 = take(n); k.c2 = take(n);
    k.cd = k.ds ? take(n) : 0;
    k.out = take(n);
    k.qm = d->save_for_backward ? take((n / 4 + 3) / 4) : 0;
    in = k.out;
  }
  if (d->save_for_backward) {
    const size_t gmax = N * p.h[2] * p.w[2] * 64;  // stage0 is the largest block tensor
    for (int j = 0; j < 4; ++j) p.G[j] = take(gmax);
    p.g0 = take(N * p.h[1] * p.w[1] * 64);
    for (int j = 0; j < NCONV; ++j) p.wg[j] = take(weights(j));
  }
  p.total = off;
  return p;
}

// ------------------------------------------------------------------ weight (un)packing
__global__ void pack_weights(const float* __restrict__ w, float* __restrict__ wf, float* __restrict__ wd, int Co, int C, int KS) {
  const int n = Co * C * KS * KS;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    // i indexes OIHW
    int r = i;
    const int kw = r % KS; r /= KS;
    const int kh = r % KS; r /= KS;
    const int c = r % C; const int co = r / C;
    const float v = w[i];
    wf[((long)(kh * KS + kw) * C + c) * Co + co] = v;
    if (wd) wd[((long)(kh * KS + kw) * Co + co) * C + c] = v;
  }
}
// all 20 convolutions' weights in ONE launch (19 separate launches of ~9 us each were 0.17 ms of a 22 ms step): the block
// index selects the convolution through a small table of block ranges.  A workgroup owns a 32 (co) x 32 (c) tile of one
// convolution: its OIHW source is 32 contiguous runs of 32*T floats, read coalesced into LDS; each of the T taps then
// leaves as a 32x32 tile whose rows are contiguous in the packed layouts (co for the forward pack, c for the dgrad pack).
// (One thread per element wrote 4-byte scatters a whole channel plane apart: 92 us for 135 MB.)
struct PackTab {
  const float* w[NCONV];
  float* wf[NCONV];
  float* wd[NCONV];      // may be null
  __bf16* wf16[NCONV];   // bf16 data path (may be null): wf16[co][(cc * T + tap) * 64 + r] = w[co][cc * 64 + r][tap]
  __bf16* wd16[NCONV];   //                               wd16[c][(cc * T + tap) * 64 + r] = w[cc * 64 + r][c][tap]
  int cout[NCONV], cin[NCONV], ks[NCONV];
  int blk0[NCONV + 1];   // first block of conv i (conv 0 = stem: one element per thread, see below)
};
constexpr int PACK_LD = 32 * 9 + 1;
__global__ void __launch_bounds__(256) pack_all(const PackTab tab) {
  __shared__ float tl[32 * PACK_LD];
  int i = 0;
#pragma unroll
  for (int j = 1; j < NCONV; ++j) i += (int)blockIdx.x >= tab.blk0[j];      // block-uniform
  const int lb = (int)blockIdx.x - tab.blk0[i];
  const float* w = tab.w[i];
  float* wf = tab.wf[i];
  if (i == 0) {     // the stem: its 3 identical input channels (Video_Net.py:64) are folded, Wf[kh*7+kw][co] = sum_c w[co][c][kh][kw]
    const int e = lb * 256 + threadIdx.x;
    if (e >= 64 * 49) return;
    const int co = e / 49, k = e % 49;
    wf[k * 64 + co] = w[(co * 3 + 0) * 49 + k] + w[(co * 3 + 1) * 49 + k] + w[(co * 3 + 2) * 49 + k];
    return;
  }
  const int Co = tab.cout[i], C = tab.cin[i], T = tab.ks[i] * tab.ks[i];     // T = 9 or 1; Co, C multiples of 32
  const int ctiles = C >> 5;
  const int co0 = (lb / ctiles) * 32, c0 = (lb % ctiles) * 32;
  const int run = 32 * T;
  for (int idx = threadIdx.x; idx < 32 * run; idx += 256) {
    const int col = idx / run, r = idx - col * run;
    tl[col * PACK_LD + r] = w[((long)(co0 + col) * C + c0) * T + r];
  }
  __syncthreads();
  float* wd = tab.wd[i];
  __bf16* wf16 = tab.wf16[i];
  __bf16* wd16 = tab.wd16[i];
  if (wf16) {     // the bf16 data path takes only these (K-contiguous rows in the GEMM's own K order; C, Co multiples of 64)
    for (int idx = threadIdx.x; idx < T * 1024; idx += 256) {
      const int tap = idx >> 10, a = (idx >> 5) & 31, b = idx & 31;
      wf16[(long)(co0 + a) * (T * C) + ((c0 >> 6) * T + tap) * 64 + (c0 & 63) + b] = (__bf16)tl[a * PACK_LD + b * T + tap];
      if (wd16) wd16[(long)(c0 + a) * (T * Co) + ((co0 >> 6) * T + tap) * 64 + (co0 & 63) + b] = (__bf16)tl[b * PACK_LD + a * T + tap];
    }
    return;
  }
  for (int idx = threadIdx.x; idx < T * 1024; idx += 256) {
    const int tap = idx >> 10, a = (idx >> 5) & 31, b = idx & 31;
    wf[((long)(tap * C + c0 + a)) * Co + co0 + b] = tl[b * PACK_LD + a * T + tap];           // row (tap, c = a), column co = b
    if (wd) wd[((long)(tap * Co + co0 + a)) * C + c0 + b] = tl[a * PACK_LD + b * T + tap];    // row (tap, co = a), column c = b
  }
}
// every convolution's packed gradient -> += the OIHW gradient, ONE launch behind the last weight-gradient GEMM (19 launches
// of ~8 us each were 0.15 ms of the step; the whole trunk is one autograd node, nobody consumes a gradient earlier)
struct UnpackTab {
  const float* pk[NCONV];
  float* dw[NCONV];        // null: this convolution's gradient is not wanted
  int cout[NCONV], cin[NCONV], ks[NCONV];
  int blk0[NCONV + 1];
};
__global__ void __launch_bounds__(256) unpack_all(const UnpackTab tab) {
  __shared__ float tl[32 * PACK_LD];
  int i = 0;
#pragma unroll
  for (int j = 1; j < NCONV; ++j) i += (int)blockIdx.x >= tab.blk0[j];      // block-uniform
  const int lb = (int)blockIdx.x - tab.blk0[i];
  float* dw = tab.dw[i];
  if (!dw) return;
  const float* pk = tab.pk[i];
  if (i == 0) {
    const int e = lb * 256 + threadIdx.x;
    if (e >= 64 * 3 * 49) return;
    dw[e] += pk[(e % 49) * 64 + e / 147];
    return;
  }
  // the mirror image of pack_all: a 32 (co) x 32 (c) tile, T taps read as rows of co, added onto 32 contiguous OIHW runs
  const int Co = tab.cout[i], C = tab.cin[i], T = tab.ks[i] * tab.ks[i];
  const int ctiles = C >> 5;
  const int co0 = (lb / ctiles) * 32, c0 = (lb % ctiles) * 32;
  for (int idx = threadIdx.x; idx < T * 1024; idx += 256) {
    const int tap = idx >> 10, a = (idx >> 5) & 31, b = idx & 31;
    tl[b * PACK_LD + a * T + tap] = pk[((long)(tap * C + c0 + a)) * Co + co0 + b];
  }
  __syncthreads();
  const int run = 32 * T;
  for (int idx = threadIdx.x; idx < 32 * run; idx += 256) {
    const int col = idx / run, r = idx - col * run;
    dw[((long)(co0 + col) * C + c0) * T + r] += tl[col * PACK_LD + r];
  }
}

// ------------------------------------------------------------------ stem convolution 7x7 / 2, 1 -> 64 channels (frames that fit LDS)
// K = 49 is two K tiles of the engine: prologue + epilogue outweighed the loop and it ran at a quarter of the output-write
// rate.  Here one workgroup owns one frame: the zero-padded frame is staged in LDS once (22 KB at 67x67), the 49x64
// weights sit in registers as MFMA B fragments, and a wave walks 32-pixel tiles: the A fragment of k-step ks is ONE
// ds_read_b32 (pixel base + tap offset: the im2col gather happens inside LDS), 25 k-steps x 2 column tiles = 50 MFMAs,
// then 32 coalesced 128-byte row stores.
__global__ void __launch_bounds__(256)
    stem_fwd_mfma(const float* __restrict__ x, const float* __restrict__ wf, float* __restrict__ y, int H, int W, int Ho, int Wo,
                  int LDW, double* __restrict__ stat) {
  // stat (may be null): BatchNorm batch statistics fused -- stat[(n * 2 + 0) * 64 + c] = sum over frame n's pixels of y[.][c],
  // [(n * 2 + 1) * 64 + c] = sum of squares (one chunk per frame; bn_finalize adds the chunks in order)
  __shared__ double red[4 * 64 * 2];
  extern __shared__ float img[];                     // (H + 6) x LDW, zero border of 3
  const int n = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int PH = H + 6;
  for (int i = threadIdx.x; i < PH * LDW; i += 256) img[i] = 0.f;
  __syncthreads();
  const float* xn = x + (long)n * H * W;
  for (int i = threadIdx.x; i < H * W; i += 256) {
    const int r = i / W, c = i - r * W;
    img[(r + 3) * LDW + c + 3] = xn[i];
  }
  float b0[25], b1[25];
  int toff[25];
#pragma unroll
  for (int ks = 0; ks < 25; ++ks) {
    const int tap = 2 * ks + lh;
    const bool live = tap < 49;
    const int tc = live ? tap : 0;
    b0[ks] = live ? wf[tc * 64 + li] : 0.f;
    b1[ks] = live ? wf[tc * 64 + 32 + li] : 0.f;
    toff[ks] = (tc / 7) * LDW + (tc % 7);
  }
  __syncthreads();
  const int npix = Ho * Wo;
  const int ntile = (npix + 31) >> 5;
  float* yn = y + (long)n * npix * 64;
  float sf0 = 0.f, qf0 = 0.f, sf1 = 0.f, qf1 = 0.f;
  for (int tile = wave; tile < ntile; tile += 4) {
    const int pix = tile * 32 + li;
    const int pc = pix < npix ? pix : 0;              // clamped: rows beyond the frame are computed and dropped
    const int ho = pc / Wo, wo = pc - ho * Wo;
    const int base = 2 * ho * LDW + 2 * wo;           // padded coordinates: input row 2*ho - 3 + 3
    float a[25];
#pragma unroll
    for (int ks = 0; ks < 25; ++ks) a[ks] = img[base + toff[ks]];
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < 25; ++ks) {
      acc0 = mfma32(a[ks], b0[ks], acc0);
      acc1 = mfma32(a[ks], b1[ks], acc1);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int p = tile * 32 + mfma32_row(r, lh);
      if (p < npix) {
        yn[(long)p * 64 + li] = acc0[r];
        yn[(long)p * 64 + 32 + li] = acc1[r];
        sf0 += acc0[r]; qf0 = fmaf(acc0[r], acc0[r], qf0);
        sf1 += acc1[r]; qf1 = fmaf(acc1[r], acc1[r], qf1);
      }
    }
  }
  if (stat == nullptr) return;
  double d[4] = {(double)sf0, (double)qf0, (double)sf1, (double)qf1};
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] += __shfl_xor(d[k], 32, 64);
  if (lh == 0) {
    red[(wave * 64 + li) * 2 + 0] = d[0]; red[(wave * 64 + li) * 2 + 1] = d[1];
    red[(wave * 64 + 32 + li) * 2 + 0] = d[2]; red[(wave * 64 + 32 + li) * 2 + 1] = d[3];
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int c = threadIdx.x;
    double a = 0, b = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { a += red[(w * 64 + c) * 2 + 0]; b += red[(w * 64 + c) * 2 + 1]; }
    stat[((long)n * 2 + 0) * 64 + c] = a;
    stat[((long)n * 2 + 1) * 64 + c] = b;
  }
}

// stem: p0 = maxpool3x3/2 pad1 ( relu(bn(c0)) ).  Also records, per pooled element, WHICH window position (dh*3+dw) holds
// the maximum -- the first one in row-major scan order, torch's rule (max_pool2d updates on a strict '>') -- so that the
// backward sends the gradient to exactly that element even when flat image regions produce exact ties.
template <bool OB = false>     // OB: p0 is stored as bf16 (the bf16 data path)
__global__ void stem_bn_relu_pool(const float* __restrict__ c0, const float* __restrict__ scale, const float* __restrict__ shift,
                                  float* __restrict__ p0, unsigned* __restrict__ am, int N, int Hc, int Wc, int Hp, int Wp) {
  const long total = (long)N * Hp * Wp * 16;  // 64 channels = 16 quads
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int q = (int)(i & 15);
    long r = i >> 4;
    const int pw = (int)(r % Wp); r /= Wp;
    const int ph = (int)(r % Hp); const int n = (int)(r / Hp);
    const float4 sc = *reinterpret_cast<const float4*>(scale + q * 4), sh = *reinterpret_cast<const float4*>(shift + q * 4);
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    unsigned idx[4] = {0, 0, 0, 0};
    for (int dh = 0; dh < 3; ++dh) {
      const int h = ph * 2 - 1 + dh;
      if ((unsigned)h >= (unsigned)Hc) continue;
      for (int dw = 0; dw < 3; ++dw) {
        const int w = pw * 2 - 1 + dw;
        if ((unsigned)w >= (unsigned)Wc) continue;
        const float4 v = *reinterpret_cast<const float4*>(c0 + ((long)(n * Hc + h) * Wc + w) * 64 + q * 4);
        const float y[4] = {fmaxf(bn_affine(v.x, sc.x, sh.x), 0.f), fmaxf(bn_affine(v.y, sc.y, sh.y), 0.f),
                            fmaxf(bn_affine(v.z, sc.z, sh.z), 0.f), fmaxf(bn_affine(v.w, sc.w, sh.w), 0.f)};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (y[k] > m[k]) { m[k] = y[k]; idx[k] = (unsigned)(dh * 3 + dw); }
      }
    }
    if constexpr (OB) store_quad_bf16(p0, i, m);
    else reinterpret_cast<float4*>(p0)[i] = make_float4(m[0], m[1], m[2], m[3]);
    if (am) am[i] = idx[0] | (idx[1] << 8) | (idx[2] << 16) | (idx[3] << 24);
  }
}

// stem backward of pool+relu: g0[n,h,w,c] = sum of dp0 over the pooled windows whose recorded arg-max is this element,
// masked by the ReLU (an all-zero window's arg-max carries no gradient).
// part (may be null; needs gridDim.x * blockDim.x % 16 == 0): the BatchNorm backward's column sums of the stem, fused -- per
// workgroup sum g0 and sum g0 * xhat per channel (what col_reduce<1> would read c0 and g0 again for), chunk = workgroup
__global__ void __launch_bounds__(256)
    stem_pool_relu_bwd(const float* __restrict__ c0, const float* __restrict__ scale, const float* __restrict__ shift,
                       const unsigned* __restrict__ am, const float* __restrict__ dp0, float* __restrict__ g0,
                       int N, int Hc, int Wc, int Hp, int Wp, const float* __restrict__ mean = nullptr,
                       const float* __restrict__ invstd = nullptr, double* __restrict__ part = nullptr) {
  __shared__ double sm[256 * 8];
  const long total = (long)N * Hc * Wc * 16;
  float s4[4] = {0.f, 0.f, 0.f, 0.f}, q4[4] = {0.f, 0.f, 0.f, 0.f};
  float mu[4] = {0.f, 0.f, 0.f, 0.f}, is[4] = {1.f, 1.f, 1.f, 1.f};
  if (part) {
    const int qc = (int)(((long)blockIdx.x * blockDim.x + threadIdx.x) & 15);
#pragma unroll
    for (int k = 0; k < 4; ++k) { mu[k] = mean[qc * 4 + k]; is[k] = invstd[qc * 4 + k]; }
  }
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int q = (int)(i & 15);
    long r = i >> 4;
    const int w = (int)(r % Wc); r /= Wc;
    const int h = (int)(r % Hc); const int n = (int)(r / Hc);
    const float4 sc = *reinterpret_cast<const float4*>(scale + q * 4), sh = *reinterpret_cast<const float4*>(shift + q * 4);
    const float4 v = reinterpret_cast<const float4*>(c0)[i];
    const bool pos[4] = {bn_affine(v.x, sc.x, sh.x) > 0.f, bn_affine(v.y, sc.y, sh.y) > 0.f, bn_affine(v.z, sc.z, sh.z) > 0.f,
                         bn_affine(v.w, sc.w, sh.w) > 0.f};
    float g[4] = {0, 0, 0, 0};
    const int ph0 = max(0, h / 2), ph1 = min(Hp - 1, (h + 1) / 2);
    const int pw0 = max(0, w / 2), pw1 = min(Wp - 1, (w + 1) / 2);
    for (int ph = ph0; ph <= ph1; ++ph)
      for (int pw = pw0; pw <= pw1; ++pw) {
        // window of (ph,pw) covers rows 2ph-1..2ph+1
        if (h < 2 * ph - 1 || h > 2 * ph + 1 || w < 2 * pw - 1 || w > 2 * pw + 1) continue;
        const unsigned me = (unsigned)((h - (2 * ph - 1)) * 3 + (w - (2 * pw - 1)));
        const long o = ((long)(n * Hp + ph) * Wp + pw) * 16 + q;
        const unsigned a = am[o];
        const float4 dp = reinterpret_cast<const float4*>(dp0)[o];
        if (pos[0] && (a & 255u) == me) g[0] += dp.x;
        if (pos[1] && ((a >> 8) & 255u) == me) g[1] += dp.y;
        if (pos[2] && ((a >> 16) & 255u) == me) g[2] += dp.z;
        if (pos[3] && (a >> 24) == me) g[3] += dp.w;
      }
    reinterpret_cast<float4*>(g0)[i] = make_float4(g[0], g[1], g[2], g[3]);
    if (part) {
      const float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) { s4[k] += g[k]; q4[k] = fmaf(g[k], (xv[k] - mu[k]) * is[k], q4[k]); }
    }
  }
  if (part == nullptr) return;
  // 256 threads = 16 row groups x 16 channel quads (thread t: quad t & 15): fixed-order sums in LDS
#pragma unroll
  for (int k = 0; k < 4; ++k) { sm[threadIdx.x * 8 + k] = (double)s4[k]; sm[threadIdx.x * 8 + 4 + k] = (double)q4[k]; }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int c = threadIdx.x, cq = c >> 2, cj = c & 3;
    double a = 0, b = 0;
    for (int l = 0; l < 16; ++l) { a += sm[(l * 16 + cq) * 8 + cj]; b += sm[(l * 16 + cq) * 8 + 4 + cj]; }
    part[((long)blockIdx.x * 2 + 0) * 64 + c] = a;
    part[((long)blockIdx.x * 2 + 1) * 64 + c] = b;
  }
}

// feat[n][c] = mean over HW of y[n][hw][c]
template <bool IB = false>     // IB: y is bf16 (the bf16 data path)
__global__ void avgpool_fwd(const float* __restrict__ y, float* __restrict__ feat, int N, int HW, int C) {
  const long total = (long)N * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C); const long n = i / C;
    float s = 0.f;
    for (int p = 0; p < HW; ++p) s += IB ? (float)reinterpret_cast<const __bf16*>(y)[(n * HW + p) * C + c] : y[(n * HW + p) * C + c];
    feat[i] = s / (float)HW;
  }
}
__global__ void avgpool_bwd(const float* __restrict__ dfeat, float* __restrict__ dy, int N, int HW, int C) {
  const long total = (long)N * HW * C;
  const float inv = 1.f / (float)HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C); const long n = i / ((long)HW * C);
    dy[i] = dfeat[n * C + c] * inv;
  }
}
__global__ void zero_f32(float* p, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = 0.f;
}

static inline int ew_grid(long n) { long b = (n + 255) / 256; return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }

// ------------------------------------------------------------------ stem weight gradient 7x7 / 2, 1 -> 64 channels
//   pk[k = kh*7 + kw][co] = sum_{n, ho, wo} x[n][2 ho - 3 + kh][2 wo - 3 + kw] * dy[n][ho][wo][co]
// On the engine this 49 x 64 x (N*Ho*Wo) product ran on scalar gathers (198 us, 37 TFLOP/s).  Here a workgroup walks whole
// frames: the zero-padded frame sits in LDS (as in stem_fwd_mfma), the contraction index is the output pixel -- lane half h
// takes pixel (ho, 2 s + h) -- so the A operand of tap (kh, kw) is the LDS word  kh*LDW + kw + 2h  +  (2 ho LDW + 4 s):
// a per-lane constant plus a wave-uniform offset, conflict-free (LDW odd), and the B operand dy[pixel][co] is a coalesced
// row.  Wave (mt, nt) owns taps 32 mt .. 32 mt + 31 (49 live) x channels 32 nt .. 32 nt + 31 in one accumulator for all its
// frames; per-workgroup sums leave through slabs and are added in workgroup order (deterministic).
constexpr int STEM_WH = 17;      // Wo / 2 of the production geometry (34 output columns); the kernel takes Wo <= 34, even
__global__ void __launch_bounds__(256)
    stem_wgrad_mfma(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ slab, int N, int H, int W,
                    int Ho, int Wo, int LDW) {
  extern __shared__ float img[];                     // (H + 6) x LDW, zero border of 3
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int mt = wave >> 1, nt = wave & 1;
  const int tap = mt * 32 + li;
  const int tc = tap < 49 ? tap : 0;                 // rows >= 49 of the accumulator are never stored
  const int abase = (tc / 7) * LDW + (tc % 7) + 2 * lh;
  const int PH = H + 6, wh = Wo >> 1;
  for (int i = threadIdx.x; i < PH * LDW; i += 256) img[i] = 0.f;      // the border stays zero for every frame
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int voff = (lh * 64 + nt * 32 + li) * 4;
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    __syncthreads();                                 // the previous frame's reads are done
    const float* xn = x + (long)n * H * W;
    for (int i = threadIdx.x; i < H * W; i += 256) {
      const int r = i / W, c = i - r * W;
      img[(r + 3) * LDW + c + 3] = xn[i];
    }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rdy = brsrc(dy + (long)n * Ho * Wo * 64, Ho * Wo * 64 * 4);
    // dy rows in batches of RB: the NEXT batch (RB x 17 loads) is in flight under this batch's RB x 17 MFMAs (~1.8 us: one
    // row ahead, 0.45 us, was shorter than the memory latency and the kernel ran 150 us instead of the engine's 198)
    constexpr int RB = 4;
    float b0[RB][STEM_WH], b1[RB][STEM_WH];
    auto rowload = [&](int ho0, float (&b)[RB][STEM_WH]) {
#pragma unroll
      for (int rr = 0; rr < RB; ++rr)
#pragma unroll
        for (int sw = 0; sw < STEM_WH; ++sw)
          b[rr][sw] = bload(rdy, (sw < wh && ho0 + rr < Ho) ? voff : BUF_OOB, ((ho0 + rr) * Wo + 2 * sw) * 256);
    };
    auto rowmul = [&](int ho0, const float (&b)[RB][STEM_WH]) {
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
        if (ho0 + rr >= Ho) break;
        const float* ap = img + abase + 2 * (ho0 + rr) * LDW;
#pragma unroll
        for (int sw = 0; sw < STEM_WH; ++sw)
          if (sw < wh) acc = mfma32(ap[4 * sw], b[rr][sw], acc);
      }
    };
    rowload(0, b0);
    for (int ho = 0; ho < Ho; ho += 2 * RB) {
      if (ho + RB < Ho) rowload(ho + RB, b1);
      __builtin_amdgcn_sched_barrier(0);
      rowmul(ho, b0);
      if (ho + RB >= Ho) break;
      if (ho + 2 * RB < Ho) rowload(ho + 2 * RB, b0);
      __builtin_amdgcn_sched_barrier(0);
      rowmul(ho + RB, b1);
    }
  }
  float* out = slab + (long)blockIdx.x * (49 * 64);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = mt * 32 + mfma32_row(r, lh);
    if (t < 49) out[t * 64 + nt * 32 + li] = acc[r];
  }
}
// pk[k][co] = sum over workgroups of slab[.][k][co], ascending: 32 elements x 8 slab groups per workgroup, combined in order
__global__ void __launch_bounds__(256) stem_wgrad_reduce(const float* __restrict__ slab, int nslab, float* __restrict__ pk) {
  __shared__ float sm[8][32];
  const int el = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + el;                // 49 * 64 = 98 * 32
  float s = 0.f;
#pragma unroll 4
  for (int b = grp; b < nslab; b += 8) s += slab[(long)b * (49 * 64) + i];
  sm[grp][el] = s;
  __syncthreads();
  if (grp != 0) return;
#pragma unroll
  for (int k = 1; k < 8; ++k) s += sm[k][el];
  pk[i] = s;
}

// ------------------------------------------------------------------ conv launchers
// gathered operands are addressed with 32-bit BYTE offsets (Ctx.boff, fetch4): at most 2^30 floats (4 GiB).  Between the
// buffer form's 2 GiB limit and this one the flat form serves; beyond it the launchers refuse (AVVAD_EINVAL).
static inline bool fits_u30(long n) { return n >= 0 && n < (1L << 30); }
// the im2col gathers keep one tap-validity bit per (kh, kw) in a 32-bit word
static inline bool taps_fit(const Geom& g) { return g.KS * g.KS <= 32; }
// operands below 2 GiB take the buffer-addressed gathers (conv_ops.h "BUF")
static inline bool fits_buf(long n_floats) { return n_floats >= 0 && n_floats < (1L << 29) - 64; }
// the stem's LDS-resident-frame kernels serve this geometry (7x7 / 2, 1 -> 64 channels, a padded frame within 48 KB of LDS)
static inline bool stem_kernel_ok(const Geom& g) {
  const int LDW = (g.W + 6) | 1;
  return g.C == 1 && g.KS == 7 && g.stride == 2 && g.pad == 3 && g.Co == 64 && (size_t)(g.H + 6) * LDW * sizeof(float) <= 48 * 1024 &&
         !avvad_tune().no_stem_kernel;
}
// (the weight-gradient kernel also wants an even output width within its register rows, and the slab for its partials)
static inline bool stem_wgrad_ok(const Geom& g, bool slab) {
  return stem_kernel_ok(g) && (g.Wo & 1) == 0 && g.Wo <= 2 * STEM_WH && slab && (long)g.Ho * g.Wo * 64 * 4 < (1L << 31);
}
// most tiles a position-class product may have (every tile is in the stream-K pool: about one split tile per worker, so the
// fix-up's traffic grows with the tile count; option "cls_cap" overrides)
static inline long cls_tile_cap() {
  if (avvad_tune().cls_cap > 0) return avvad_tune().cls_cap;
  return 4L * grid_cus();     // (measured: 2/CU -> 4/CU: step -0.07 ms)
}
// ---- position classes (igemm.h): 3x3 / pad 1 convolutions whose tile count fits the stream-K pool skip the zero padding
static inline bool cls_common(const Geom& g, bool slab) {
  return avvad_tune().bf16 == 0 && !avvad_tune().no_cls && slab && g.KS == 3 && g.pad == 1 && g.N >= 128 && g.C % 32 == 0 &&
         g.Co % 32 == 0 && g.Ho >= 2 && g.Wo >= 2 && avvad_tune().igemm_variant < 0 && !avvad_tune().no_buf &&
         avvad_tune().no_streamk == 0;
}
static inline bool conv_fwd_cls_ok(const Geom& g, bool slab) {
  if (!cls_common(g, slab) || g.Co % 4 || g.Co < 128) return false;
  const long tiles = (long)g.Ho * g.Wo * cdiv(g.N, 128) * cdiv(g.Co, 128);
  return tiles <= cls_tile_cap() &&
         fits_buf((long)g.N * g.H * g.W * g.C) && fits_buf(9L * g.C * g.Co);
}
static inline bool conv_dgrad_cls_ok(const Geom& g, bool slab) {
  // (stride 2: the parity classes as position classes of ONE product, igemm::ClassSched::s2, instead of four accumulating launches
  //  over a zero-filled dx; option no_s2_cls keeps the four launches)
  if (!cls_common(g, slab) || (g.stride != 1 && (g.stride != 2 || avvad_tune().no_s2_cls)) || g.C % 4 || g.C < 128) return false;
  const long tiles = (long)g.H * g.W * cdiv(g.N, 128) * cdiv(g.C, 128);
  return tiles <= cls_tile_cap() &&
         fits_buf((long)g.N * g.Ho * g.Wo * g.Co) && fits_buf(9L * g.C * g.Co);
}
// weight gradient by taps (igemm.h TapSched): only the grid positions at which a tap is inside the image are contracted
static inline bool conv_wgrad_tap_ok(const Geom& g, bool slab) {
  if (!cls_common(g, slab) || g.C % 128 || g.Co % 4 || g.Co < 128) return false;
  return 9L * (g.C / 128) * cdiv(g.Co, 128) <= cls_tile_cap() &&
         fits_buf((long)g.N * g.H * g.W * g.C) && fits_buf((long)g.N * g.Ho * g.Wo * g.Co);
}
// ---- the 64 -> 64 channel 3x3 / 1 / 1 convolutions (ResNet layer1): weights-stationary kernel, conv64.h.  The fp32 form
// also wants option bf16 at 0; the bf16 form (conv64::kernel<conv64::B16, .>) serves the bf16 data path whatever the option
static inline bool conv64_ok(const Geom& g, bool b16) {
  const long M = (long)g.N * g.H * g.W;
  return (b16 || avvad_tune().bf16 == 0) && !avvad_tune().no_conv64 && g.C == 64 && g.Co == 64 && g.KS == 3 && g.stride == 1 &&
         g.pad == 1 && g.Ho == g.H && g.Wo == g.W && M > 0 && fits_buf(M * 64) &&
         (unsigned long)(M + 64) * (unsigned long)(g.H * g.W) < 0x100000000ull;
}
// (the weight gradient: output-stationary kernel + ordered reduction of the per-CU partials)
static inline bool conv64_wgrad_ok(const Geom& g, bool slab) {
  return conv64_ok(g, false) && slab && g.W <= conv64::WG_MAXW && (size_t)grid_cus() * conv64::WG_PART <= igemm::SLAB_FLOATS &&
         (long)g.N * g.H * g.W * 256 < (1L << 31);
}

// ---- the bf16 data path (option "bf16" = 1; bgemm.h)
// Operands are bf16 in HBM: activations / output gradients NHWC bf16 (written by the BatchNorm elementwise kernels), weights
// in the K-contiguous bf16 packs of pack_all.  Outputs are fp32 (raw convolution sums feed BatchNorm statistics; gradients
// accumulate).  Channel counts must be multiples of 64 (every trunk convolution behind the stem), operands < 2 GiB.
static inline bool native_bf16() { return avvad_tune().bf16 == 1; }
static inline bool bf16_conv_ok(const Geom& g) {
  return g.C % 64 == 0 && g.Co % 64 == 0 && taps_fit(g) && fits_buf((long)g.N * g.H * g.W * g.C / 2) &&
         fits_buf((long)g.N * g.Ho * g.Wo * g.Co / 2) && fits_buf((long)g.KS * g.KS * g.C * g.Co / 2);
}
// position classes on the bf16 engine (the zero padding skipped: igemm.h); 64-channel chunks
// (the bf16 kernels are bound by operand traffic, not by the matrix pipe: skipped products buy time only where they are 40 %
//  of the tile -- the 3x3 grid -- and on larger grids the all-tiles-in-the-pool fix-up costs more than they save: measured
//  per forward launch, 9x9 grid 55 -> 74 us, 5x5 66 -> 73 us, 3x3 78 -> 65 us)
static inline bool cls16_common(const Geom& g, bool slab) {
  return !avvad_tune().no_cls && slab && g.KS == 3 && g.pad == 1 && g.N >= 128 && g.Ho >= 2 && g.Wo >= 2 && g.Ho * g.Wo <= 9 &&
         avvad_tune().no_streamk == 0;
}
static inline bool conv_fwd16_cls_ok(const Geom& g, bool slab) {
  if (!cls16_common(g, slab) || g.Co < 128) return false;
  return (long)g.Ho * g.Wo * cdiv(g.N, 128) * cdiv(g.Co, 128) <= cls_tile_cap();
}
// stride 2, 3x3: the four parity classes as position classes of ONE product (igemm::ClassSched::s2) -- on this engine the four
// separate launches are ~40 us each whatever their size, so grouping pays on every grid (unlike the stride-1 classes)
static inline bool conv_dgrad16_cls_ok(const Geom& g, bool slab) {
  const bool form = g.stride == 1 ? cls16_common(g, slab)
                                  : g.stride == 2 && g.KS == 3 && g.pad == 1 && !avvad_tune().no_cls && !avvad_tune().no_s2_cls &&
                                        avvad_tune().no_streamk == 0 && slab && g.N >= 128;
  return form && g.C >= 128 && (long)g.H * g.W * cdiv(g.N, 128) * cdiv(g.C, 128) <= cls_tile_cap();
}
static inline bool conv_wgrad16_tap_ok(const Geom& g, bool slab) {
  return cls16_common(g, slab) && g.C % 128 == 0 && g.Co >= 128 && 9L * (g.C / 128) * cdiv(g.Co, 128) <= cls_tile_cap();
}

// ---- which kernel form runs a convolution: one choice per direction and data path, made at every call (the backward runs
// under BwdCuCap, whose lower max_cus changes cls_tile_cap() and grid_cus()).  The launchers switch on it, and the forward's
// BatchNorm statistics read from it how many partial-sum chunks the epilogue leaves.
// STEM: the stem's LDS-resident-frame kernels.  CONV64: conv64.h.  CLS: position classes (igemm.h; the stride-2 data gradient
// as one product over its parity classes).  TAP: the weight gradient by taps (igemm.h TapSched).  PARITY: the stride-2 data
// gradient as four parity-class GEMMs (conv_ops.h).  ENGINE: the im2col engine (with the stem's own gathers when C == 1).
enum Form { STEM, CONV64, CLS, TAP, PARITY, ENGINE };
struct ConvForm {
  Form form;
  int rows, cols;   // ENGINE / PARITY: the engine's tile
  bool buf;         // ENGINE / PARITY: buffer-addressed gathers (the bf16 engine's always are)
  int chunks;       // forward: partial-sum chunks of the column statistics its epilogue leaves in `stat` (0: none)
};
static ConvForm fwd_form(const Geom& g, bool b16, bool slab) {
  const long M = (long)g.N * g.Ho * g.Wo;
  const int cols = g.Co <= 64 ? 64 : 128;
  if (conv64_ok(g, b16)) return {CONV64, 0, 0, false, conv64::grid_for((long)g.N * g.H * g.W, grid_cus())};   // one per workgroup
  if (b16 ? conv_fwd16_cls_ok(g, slab) : conv_fwd_cls_ok(g, slab)) return {CLS, 0, 0, false, g.Ho * g.Wo * cdiv(g.N, 128)};
  if (b16) return {ENGINE, 128, cols, true, cdiv(M, 128)};
  if (g.C == 1) return stem_kernel_ok(g) ? ConvForm{STEM, 0, 0, false, g.N} : ConvForm{ENGINE, 128, 64, false, 0};   // (per frame)
  const int rows = g.Co <= 64 && !avvad_tune().no_tall ? 256 : 128;
  const bool buf = fits_buf((long)g.N * g.H * g.W * g.C) && fits_buf((long)g.KS * g.KS * g.C * g.Co) && !avvad_tune().no_buf;
  return {ENGINE, rows, cols, buf, cdiv(M, rows)};
}
static ConvForm dgrad_form(const Geom& g, bool b16, bool slab) {
  if (conv64_ok(g, b16)) return {CONV64};
  if (b16 ? conv_dgrad16_cls_ok(g, slab) : conv_dgrad_cls_ok(g, slab)) return {CLS};
  const int cols = g.C <= 64 ? 64 : 128;
  const bool buf = b16 || (fits_buf((long)g.N * g.Ho * g.Wo * g.Co) && fits_buf((long)g.KS * g.KS * g.C * g.Co) && !avvad_tune().no_buf);
  if (g.stride == 2) return {PARITY, 128, cols, buf};
  return {ENGINE, cols == 64 && !b16 && !avvad_tune().no_tall ? 256 : 128, cols, buf};
}
static ConvForm wgrad_form(const Geom& g, bool b16, bool slab) {
  const int cols = g.Co <= 64 ? 64 : 128;
  if (b16) return conv_wgrad16_tap_ok(g, slab) ? ConvForm{TAP} : ConvForm{ENGINE, 128, cols, true};
  if (conv64_wgrad_ok(g, slab)) return {CONV64};
  if (conv_wgrad_tap_ok(g, slab)) return {TAP};
  if (g.C == 1) return stem_wgrad_ok(g, slab) ? ConvForm{STEM} : ConvForm{ENGINE, 64, 64, false};
  const bool buf = fits_buf((long)g.N * g.H * g.W * g.C) && fits_buf((long)g.N * g.Ho * g.Wo * g.Co) && !avvad_tune().no_buf;
  return {ENGINE, 128, cols, buf};
}

// ---- the schedules the launchers share between the data paths (K chunk kc: 32 channels fp32, 64 bf16)
static igemm::ClassSched fwd_sched(const Geom& g, int kc) {
  const int lsh = ((g.Ho - 1) * g.stride - g.pad + 2 > g.H - 1) ? 1 : 0, lsw = ((g.Wo - 1) * g.stride - g.pad + 2 > g.W - 1) ? 1 : 0;
  return igemm::ClassSched{g.Ho, g.Wo, cdiv(g.Co, 128), g.C / kc, cdiv(g.N, 128), 3, 1, lsh, 1, lsw};
}
static igemm::ClassSched dgrad_sched(const Geom& g, int kc) {
  igemm::ClassSched sc{g.H, g.W, cdiv(g.C, 128), g.Co / kc, cdiv(g.N, 128), 3, 1, 1, 1, 1};
  if (g.stride == 2) { sc.s2 = 1; sc.Hq = g.Ho; sc.Wq = g.Wo; }
  return sc;
}
static inline igemm::TapSched tap_sched(const Geom& g, int tiles_per_tap) {
  const int NP = cdiv(g.N, 128) * 128;
  const int lsh = ((g.Ho - 1) * g.stride - g.pad + 2 > g.H - 1) ? 1 : 0, lsw = ((g.Wo - 1) * g.stride - g.pad + 2 > g.W - 1) ? 1 : 0;
  return igemm::TapSched{g.Ho, g.Wo, tiles_per_tap, NP / 32, 3, 1, lsh, 1, lsw};
}

// ---- what the data paths do differently, in one place.  The launchers below are one text per direction and kernel form; B16
// selects the bf16 data path (bgemm.h): its operands are bf16 PAIRS behind float pointers, so the gathers see a geometry with
// half the channels; its weights are the K-contiguous packs (RowPairs*); its K chunk is 64 channels; its gathers always take
// the buffer form; its engine has 128-row tiles only, takes no split-K hint, and wants to be told when K runs over pixels (MM).
template <bool B16> constexpr int KCH = B16 ? 64 : 32;     // channels per K chunk of the class schedules
template <bool B16> constexpr int UNIT = B16 ? 2 : 1;      // elements per operand unit
template <bool B16>
static Geom unit_geom(Geom g, bool c, bool co) {           // the geometry a gather sees: g with C and / or Co in operand units
  if (c) g.C /= UNIT<B16>;
  if (co) g.Co /= UNIT<B16>;
  return g;
}
// B operand of a forward (n = Co, cin = C) or data-gradient (n = C, cin = Co) product: the rows of the weight pack
template <bool B16, bool BUF>
static auto weight_rows(const float* w, int n, int cin, int T) {
  if constexpr (B16) return bgemm::RowPairs{w, T * cin / 2, n, T * cin / 2};
  else return convop::ColTapRows<BUF>{w, n, n, T * cin, cin, T, convop::div_magic(T)};
}
// ... for the live taps of a tile's position class (3x3; flip: the data gradient)
template <bool B16>
static auto weight_rows_cls(const float* w, int n, int cin, int flip, const igemm::ClassRow& cr, const igemm::ClassSched& sc) {
  if constexpr (B16) return bgemm::RowPairsCls{w, 9 * cin / 2, n, 9, 3, flip, cr, sc};
  else return convop::ColTapRowsCls{w, n, n, cin, 3, flip, cr, sc};
}
template <bool B16, bool MM = false, class A, class B, class E>
static int cls_launch(const A& a, const B& b, const E& e, int Mp, int N, hipStream_t s, float* slab) {
  if constexpr (B16) return bgemm::launch_cls<MM>(a, b, e, Mp, N, s, slab);
  else return igemm::launch_cls(a, b, e, Mp, N, s, slab);
}
// the ENGINE / PARITY forms' tile dispatch (TALL: this product has the fp32 engine's 256-row instantiation; K in operand units)
template <bool B16, bool TALL, bool MM = false, class A, class B, class E>
static int tile_launch(const ConvForm& f, const A& a, const B& b, const E& e, int M, int N, int K, int split, hipStream_t s, float* slab) {
  if constexpr (B16) {
    if (f.cols == 64) return bgemm::launch<128, 64, MM>(a, b, e, M, N, K, s, slab);
    return bgemm::launch<128, 128, MM>(a, b, e, M, N, K, s, slab);
  } else {
    if constexpr (TALL)
      if (f.rows == 256) return igemm::launch<256, 64>(a, b, e, M, N, K, split, s, slab);
    if (f.cols == 64) return igemm::launch<128, 64>(a, b, e, M, N, K, split, s, slab);
    return igemm::launch<128, 128>(a, b, e, M, N, K, split, s, slab);
  }
}

// y = conv(x) (flip = false, wpk = forward pack) or dx (+)= dgrad(dy) (flip = true, wpk = dgrad pack); b16: bf16 activations /
// packs in (conv64::B16), fp32 out
static int conv64_launch(bool b16, bool flip, const float* x, const float* wpk, float* y, const Geom& g, int accumulate, hipStream_t s,
                         double* stat) {
  const int M = g.N * g.H * g.W;
  const int grid = conv64::grid_for(M, grid_cus());
  const unsigned mg_hw = convop::div_magic((unsigned)(g.H * g.W)), mg_w = convop::div_magic((unsigned)g.W);
  auto k = b16 ? (flip ? conv64::kernel<conv64::B16, true> : conv64::kernel<conv64::B16, false>)
               : (flip ? conv64::kernel<conv64::F32, true> : conv64::kernel<conv64::F32, false>);
  hipLaunchKernelGGL(k, dim3(grid), dim3(conv64::NW * 64), 0, s, x, wpk, y, M, g.H, g.W, mg_hw, mg_w, accumulate, stat);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

// ---- forward: y = conv(x).  b16: x and the pack wf are bf16.  stat: the column sums / sums of squares of y for the fused
// BatchNorm statistics, one chunk per ConvForm::chunks (igemm::EpiStore::stat), or null
template <bool B16>
static int conv_fwd_cls(const float* x, const float* wf, float* y, const Geom& g, hipStream_t s, float* slab, double* stat) {
  const int MB = cdiv(g.N, 128), P = g.Ho * g.Wo;
  const igemm::ClassSched sc = fwd_sched(g, KCH<B16>);
  const igemm::ClassRow cr{P, convop::div_magic(P)};
  convop::Im2colFwdCls a{x, unit_geom<B16>(g, true, false), g.N, cr, sc};
  const auto b = weight_rows_cls<B16>(wf, g.Co, g.C, 0, cr, sc);
  igemm::EpiCls e{y, (long)P * g.Co, nullptr, 0};
  e.stat = stat; e.W = g.Co; e.rows = g.N; e.cr = cr; e.sched = sc;
  return cls_launch<B16>(a, b, e, MB * P * 128, g.Co, s, slab);
}
template <bool B16, bool BUF>
static int conv_fwd_engine(const float* x, const float* wf, float* y, const Geom& g, const ConvForm& f, hipStream_t s, float* slab,
                           double* stat) {
  const int M = g.N * g.Ho * g.Wo, T = g.KS * g.KS, K = T * g.C;
  igemm::EpiStore e{y, g.Co, nullptr, 0};
  if constexpr (!B16) {
    if (g.Co % 4) return AVVAD_EINVAL;                         // ColPlain<4> / ColTapRows fetch 16 bytes of a weight row
    if (g.C == 1) {                                            // the stem's own operands
      igemm::ColPlain<4> b{wf, g.Co, g.Co, K, 0};
      convop::StemFwd a{x, g, M, K};
      return igemm::launch<128, 64>(a, b, e, M, g.Co, K, 1, s, slab);
    }
    if (g.C % 32 || g.Co % 4 || !taps_fit(g)) return AVVAD_EINVAL;
    if (!fits_u30((long)g.N * g.H * g.W * g.C) || !fits_u30((long)K * g.Co)) return AVVAD_EINVAL;   // 32-bit BYTE offsets in the gathers
  }
  e.stat = stat;
  convop::Im2colFwd<BUF> a{x, unit_geom<B16>(g, true, false), M, convop::tap_div(T, g.KS)};
  const auto b = weight_rows<B16, BUF>(wf, g.Co, g.C, T);
  return tile_launch<B16, true>(f, a, b, e, M, g.Co, K / UNIT<B16>, 1, s, slab);
}
static int conv_fwd(bool b16, const float* x, const float* wf, float* y, const Geom& g, hipStream_t s, float* slab, double* stat = nullptr) {
  if (b16 && !bf16_conv_ok(g)) return AVVAD_EINVAL;
  const ConvForm f = fwd_form(g, b16, slab);
  switch (f.form) {
    case STEM: {
      const int LDW = (g.W + 6) | 1;
      hipLaunchKernelGGL(stem_fwd_mfma, dim3(g.N), dim3(256), (size_t)(g.H + 6) * LDW * sizeof(float), s, x, wf, y, g.H, g.W, g.Ho, g.Wo,
                         LDW, stat);
      AVVAD_LAUNCH_CHECK();
      return AVVAD_OK;
    }
    case CONV64: return conv64_launch(b16, false, x, wf, y, g, 0, s, stat);
    case CLS: return b16 ? conv_fwd_cls<true>(x, wf, y, g, s, slab, stat) : conv_fwd_cls<false>(x, wf, y, g, s, slab, stat);
    default:
      if (b16) return conv_fwd_engine<true, true>(x, wf, y, g, f, s, slab, stat);
      return f.buf ? conv_fwd_engine<false, true>(x, wf, y, g, f, s, slab, stat) : conv_fwd_engine<false, false>(x, wf, y, g, f, s, slab, stat);
  }
}

// ---- data gradient: dx (+)= dgrad(dy).  b16: dy and the pack wd are bf16
template <bool B16>
static int conv_dgrad_cls(const float* dy, const float* wd, float* dx, const Geom& g, int accumulate, hipStream_t s, float* slab) {
  const int MB = cdiv(g.N, 128), P = g.H * g.W;
  const igemm::ClassSched sc = dgrad_sched(g, KCH<B16>);
  const igemm::ClassRow cr{P, convop::div_magic(P)};
  convop::Im2colDgradCls a{dy, unit_geom<B16>(g, false, true), g.N, cr, sc};
  const auto b = weight_rows_cls<B16>(wd, g.C, g.Co, 1, cr, sc);
  igemm::EpiCls e{dx, (long)P * g.C, nullptr, accumulate ? 1 : 0};
  e.W = g.C; e.rows = g.N; e.cr = cr; e.sched = sc;
  return cls_launch<B16>(a, b, e, MB * P * 128, g.C, s, slab);
}
// stride-2 data gradient by parity classes (conv_ops.h): per class (ph, pw) of input positions, one small GEMM over the taps
// that reach it, accumulating into dx.  gemm(c, Mc, ntap, e) launches class c's.
template <class Gemm>
static int dgrad_parity(float* dx, const Geom& g, int accumulate, hipStream_t s, Gemm gemm) {
  const long n = (long)g.N * g.H * g.W * g.C;
  const auto cls = [&](int ph, int pw) {
    convop::S2Class c;
    c.ph = ph; c.pw = pw;
    c.Hc = (g.H - ph + 1) / 2; c.Wc = (g.W - pw + 1) / 2;
    c.kh0 = (ph + g.pad) & 1; c.kw0 = (pw + g.pad) & 1;
    c.nkh = c.kh0 < g.KS ? (g.KS - c.kh0 + 1) / 2 : 0;
    c.nkw = c.kw0 < g.KS ? (g.KS - c.kw0 + 1) / 2 : 0;
    c.oh = (ph + g.pad - c.kh0) / 2; c.ow = (pw + g.pad - c.kw0) / 2;
    c.mg_ntap = c.mg_nkw = 0u;
    return c;
  };
  // every refusal comes before the first launch: a refused call leaves dx as it was
  for (int q = 0; q < 4; ++q) {
    const convop::S2Class c = cls(q >> 1, q & 1);
    const int Mc = g.N * c.Hc * c.Wc, ntap = c.nkh * c.nkw;
    if (Mc <= 0 || ntap <= 0) continue;
    if (ntap > 4) return AVVAD_EINVAL;
    if ((unsigned long)(Mc + 128) * (unsigned long)(c.Hc * c.Wc) >= 0x100000000ull) return AVVAD_EINVAL;   // fast_div range
  }
  if (!accumulate) hipLaunchKernelGGL(zero_f32, dim3(ew_grid(n)), dim3(256), 0, s, dx, n);
  for (int ph = 0; ph < 2; ++ph)
    for (int pw = 0; pw < 2; ++pw) {
      convop::S2Class c = cls(ph, pw);
      const int Mc = g.N * c.Hc * c.Wc, ntap = c.nkh * c.nkw;
      if (Mc <= 0 || ntap <= 0) continue;
      c.mg_ntap = convop::div_magic(ntap); c.mg_nkw = convop::div_magic(c.nkw);
      const convop::EpiS2 e{dx, g.C, nullptr, 1, 1, g.H, g.W, c.Hc, c.Wc, ph, pw, convop::div_magic(c.Hc * c.Wc), convop::div_magic(c.Wc)};
      if (const int rc = gemm(c, Mc, ntap, e)) return rc;
    }
  return AVVAD_OK;
}
// (the ENGINE and PARITY forms)
template <bool B16, bool BUF>
static int conv_dgrad_engine(const float* dy, const float* wd, float* dx, const Geom& g, const ConvForm& f, int accumulate, hipStream_t s,
                             float* slab) {
  const int M = g.N * g.H * g.W, T = g.KS * g.KS, K = T * g.Co;
  if constexpr (!B16) {
    if (g.Co % 32 || g.C % 4 || !taps_fit(g)) return AVVAD_EINVAL;
    if (!fits_u30((long)g.N * g.Ho * g.Wo * g.Co) || !fits_u30((long)K * g.C)) return AVVAD_EINVAL;   // 32-bit BYTE offsets in the gathers
  }
  const Geom gu = unit_geom<B16>(g, false, true);
  if (f.form == PARITY)
    return dgrad_parity(dx, g, accumulate, s, [&](const convop::S2Class& c, int Mc, int ntap, const convop::EpiS2& e) {
      const int Kc = ntap * g.Co / UNIT<B16>;
      convop::Im2colDgradS2<BUF> a{dy, gu, c, Mc};
      auto b = [&] {      // the class's taps: their K positions in the bf16 pack, their first rows in the fp32 one
        if constexpr (B16) return bgemm::RowPairsSeg{wd, K / 2, g.C, Kc, T, ntap, {0, 0, 0, 0}, convop::div_magic(ntap)};
        else return convop::ColSegRows<BUF>{wd, g.C, g.C, Kc, ntap, {0, 0, 0, 0}, convop::div_magic(ntap)};
      }();
      for (int ia = 0; ia < c.nkh; ++ia)
        for (int ib = 0; ib < c.nkw; ++ib) {
          const int tap = (c.kh0 + 2 * ia) * g.KS + (c.kw0 + 2 * ib);
          if constexpr (B16) b.tap[ia * c.nkw + ib] = tap;
          else b.rowbase[ia * c.nkw + ib] = tap * g.Co;
        }
      return tile_launch<B16, false>(f, a, b, e, Mc, g.C, Kc, 1, s, slab);
    });
  igemm::EpiStore e{dx, g.C, nullptr, accumulate ? 1 : 0};
  convop::Im2colDgrad<BUF> a{dy, gu, M, convop::tap_div(T, g.KS)};
  const auto b = weight_rows<B16, BUF>(wd, g.C, g.Co, T);
  return tile_launch<B16, true>(f, a, b, e, M, g.C, K / UNIT<B16>, 1, s, slab);
}
static int conv_dgrad(bool b16, const float* dy, const float* wd, float* dx, const Geom& g, int accumulate, hipStream_t s, float* slab) {
  if (b16 && !bf16_conv_ok(g)) return AVVAD_EINVAL;
  const ConvForm f = dgrad_form(g, b16, slab);
  switch (f.form) {
    case CONV64: return conv64_launch(b16, true, dy, wd, dx, g, accumulate, s, nullptr);
    case CLS: return b16 ? conv_dgrad_cls<true>(dy, wd, dx, g, accumulate, s, slab) : conv_dgrad_cls<false>(dy, wd, dx, g, accumulate, s, slab);
    default:      // PARITY, ENGINE
      if (b16) return conv_dgrad_engine<true, true>(dy, wd, dx, g, f, accumulate, s, slab);
      return f.buf ? conv_dgrad_engine<false, true>(dy, wd, dx, g, f, accumulate, s, slab)
                   : conv_dgrad_engine<false, false>(dy, wd, dx, g, f, accumulate, s, slab);
  }
}

// ---- weight gradient: pk[(kh,kw,c)][co] = wgrad (overwritten; tiles split along K are combined by the engine's fix-up kernel,
// in a fixed order).  b16: x and dy are bf16
template <bool B16>
static int conv_wgrad_tap(const float* x, const float* dy, float* pk, const Geom& g, hipStream_t s, float* slab) {
  const int M = 9 * g.C;
  const igemm::TapSched sc = tap_sched(g, (g.C / 128) * cdiv(g.Co, 128));
  const Geom gu = unit_geom<B16>(g, true, true);
  convop::WgradXTap a{x, gu, M / UNIT<B16>, g.C, g.N, convop::div_magic(gu.C), sc};
  convop::ColDyTap b{dy, gu, gu.Co, g.C, g.N, sc};
  igemm::EpiTap e{pk, g.Co, nullptr, 0};
  e.Mrows = M; e.sched = sc;
  return cls_launch<B16, true>(a, b, e, M, g.Co, s, slab);
}
template <bool B16, bool BUF>
static int conv_wgrad_engine(const float* x, const float* dy, float* pk, const Geom& g, const ConvForm& f, hipStream_t s, float* slab) {
  const int T = g.KS * g.KS, M = T * g.C, K = g.N * g.Ho * g.Wo;
  // ColPlain<4> fetches 16 bytes of a dy row: with Co % 4 != 0 the last fetch of a row runs into the next one and, in the last
  // row, past the operand's end (the bf16 path's Co % 64 == 0 is checked by bf16_conv_ok)
  if (!B16 && g.Co % 4) return AVVAD_EINVAL;
  igemm::ColPlain<4, BUF> b{dy, g.Co / UNIT<B16>, g.Co / UNIT<B16>, K, 0};
  int split = 1;                                               // (the fp32 engine's split-K hint)
  if constexpr (!B16) {
    const int ktiles = cdiv(K, igemm::BK);
    if (g.C == 1) {                                            // the stem's own operands
      igemm::EpiStore e{pk, g.Co, nullptr, 0};
      convop::StemWgradX a{x, g, M, K};
      split = 1024; if (split > ktiles) split = ktiles;
      return igemm::launch<64, 64>(a, b, e, M, g.Co, K, split, s, slab);
    }
    if (g.C % 32) return AVVAD_EINVAL;
    if ((unsigned long)(K + igemm::BK) * (unsigned long)(g.Ho * g.Wo) >= 0x100000000ull) return AVVAD_EINVAL;   // fast_div range
    if (!fits_u30((long)g.N * g.H * g.W * g.C) || !fits_u30((long)K * g.Co)) return AVVAD_EINVAL;                // 32-bit BYTE offsets in the gathers
    const int nb = cdiv(M, 128) * cdiv(g.Co, f.cols);
    split = cdiv(1024, nb); if (split > ktiles) split = ktiles;
  }
  convop::EpiWgrad e{pk, g.Co, nullptr, 0, 1, g.C, T, convop::div_magic(T), B16 ? 6 : 5};     // (log2 of the K chunk's channels)
  convop::WgradX<BUF> a{x, unit_geom<B16>(g, true, false), M / UNIT<B16>, K, convop::div_magic(g.Ho * g.Wo), convop::div_magic(g.Wo)};
  return tile_launch<B16, false, true>(f, a, b, e, M, g.Co, K, split, s, slab);
}
static int conv_wgrad(bool b16, const float* x, const float* dy, float* pk, const Geom& g, hipStream_t s, float* slab) {
  if (b16) {
    const int K = g.N * g.Ho * g.Wo;
    if (!bf16_conv_ok(g)) return AVVAD_EINVAL;
    if ((unsigned long)(K + bgemm::BKU) * (unsigned long)(g.Ho * g.Wo) >= 0x100000000ull) return AVVAD_EINVAL;   // fast_div range
  }
  const ConvForm f = wgrad_form(g, b16, slab);
  switch (f.form) {
    case STEM: {
      const int LDW = (g.W + 6) | 1;
      const int nb = g.N < 256 ? g.N : 256;                       // one workgroup per CU, whole frames each
      hipLaunchKernelGGL(stem_wgrad_mfma, dim3(nb), dim3(256), (size_t)(g.H + 6) * LDW * sizeof(float), s, x, dy, slab, g.N, g.H, g.W,
                         g.Ho, g.Wo, LDW);
      hipLaunchKernelGGL(stem_wgrad_reduce, dim3(49 * 64 / 32), dim3(256), 0, s, slab, nb, pk);
      AVVAD_LAUNCH_CHECK();
      return AVVAD_OK;
    }
    case CONV64: {      // (fp32 only: output-stationary kernel + ordered reduction of the per-CU partials)
      const int NR = g.N * g.H;
      const int grid = NR < grid_cus() ? NR : grid_cus();
      hipLaunchKernelGGL(conv64::wgrad_kernel, dim3(grid), dim3(conv64::WG_WAVES * 64), 0, s, x, dy, slab, NR, g.H, g.W,
                         convop::div_magic((unsigned)g.H));
      hipLaunchKernelGGL(conv64::wgrad_reduce, dim3(conv64::WG_PART / 256), dim3(256), 0, s, (const float*)slab, grid, pk);
      AVVAD_LAUNCH_CHECK();
      return AVVAD_OK;
    }
    case TAP: return b16 ? conv_wgrad_tap<true>(x, dy, pk, g, s, slab) : conv_wgrad_tap<false>(x, dy, pk, g, s, slab);
    default:
      if (b16) return conv_wgrad_engine<true, true>(x, dy, pk, g, f, s, slab);
      return f.buf ? conv_wgrad_engine<false, true>(x, dy, pk, g, f, s, slab) : conv_wgrad_engine<false, false>(x, dy, pk, g, f, s, slab);
  }
}

// ------------------------------------------------------------------ one run of the trunk: what every step of a forward or backward needs
constexpr const float* NOF = nullptr;      // an optional float operand that is absent, as a typed kernel argument
struct BnSlots { float *scale, *shift, *mean, *invstd; };      // one convolution's BatchNorm: the forward's affine map, its batch statistics
struct Run {
  const Plan& p;
  float* ws;
  const avvad_trunk_params* prm;
  const avvad_trunk_grads* g;      // (the backward's; null in a forward)
  const avvad_trunk_desc* d;
  hipStream_t s;
  float* at(size_t off) const { return ws + off; }
  double* part() const { return reinterpret_cast<double*>(ws + p.part); }      // the column statistics' partial sums
  BnSlots bn(int i) const {      // conv i's slots
    const size_t o = (size_t)i * MAXC;
    return {at(p.bn_scale + o), at(p.bn_shift + o), at(p.bn_mean + o), at(p.bn_invstd + o)};
  }
  long rows(int i) const { const Geom& g = p.geom[i]; return (long)g.N * g.Ho * g.Wo; }      // pixels of conv i's output
};

struct StatCtx { int nchunk; long rows_per_chunk; };
static StatCtx stat_ctx(long M, int C) {
  const int RL = 256 / (C / 4);
  long per = (M + STAT_CHUNKS - 1) / STAT_CHUNKS;
  if (per < 16L * RL) per = 16L * RL;   // >= 16 rows per thread: fewer, fuller chunks for the small deep layers (the finalize
                                         // kernels read every chunk's partial sums)
  per = (per + RL - 1) / RL * RL;
  return {cdiv(M, per), per};
}

// partial-sum chunks of conv i's batch statistics that its forward leaves in the partial-sum buffer (the form's: one per M tile of
// its GEMM, per conv64 workgroup, per stem frame), 0: the separate column-reduction pass forms them
static int fused_chunks(const Run& r, int i, bool b16) {
  if (!r.d->training || avvad_tune().no_fused_stats) return 0;
  const int n = fwd_form(r.p.geom[i], b16, true).chunks;
  return (long)n * r.p.geom[i].Co <= (long)STAT_CHUNKS * MAXC ? n : 0;      // the partial-sum buffer's size
}
// batch statistics of conv output i -> scale/shift/mean/invstd slots i (+ running stats).  fused: the chunks its forward left
static int bn_prepare(const Run& r, int i, const float* craw, int fused) {
  const int C = r.p.geom[i].Co;
  const long M = r.rows(i);
  StatCtx sc = stat_ctx(M, C);
  if (fused) {
    sc.nchunk = fused;
  } else if (r.d->training) {
    hipLaunchKernelGGL(col_reduce<0>, dim3(sc.nchunk), dim3(256), 0, r.s, craw, NOF, NOF, NOF, NOF, M, C, sc.rows_per_chunk, r.part());
  }
  const BnSlots bn = r.bn(i);
  hipLaunchKernelGGL(bn_finalize, dim3(cdiv(C, FIN_CH)), dim3(256), 0, r.s, r.part(), sc.nchunk, M, C, r.prm->bn_w[i], r.prm->bn_b[i],
                     r.prm->bn_rm[i], r.prm->bn_rv[i], r.d->training, r.d->momentum, r.d->eps, bn.scale, bn.shift, bn.mean, bn.invstd);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
// forward of conv i and its BatchNorm's statistics: y = conv(x), then slots i.  Whether the convolution's epilogue leaves the
// statistics' partial sums is decided here, once, for both launches.  (The stem is fp32 on either data path.)
static int conv_bn(const Run& r, int i, const float* x, float* y) {
  const bool b16 = i > 0 && native_bf16();
  const int fused = fused_chunks(r, i, b16);
  const float* wf = r.at(b16 ? r.p.wf16[i] : r.p.wf[i]);
  if (const int rc = conv_fwd(b16, x, wf, y, r.p.geom[i], r.s, r.at(r.p.slab), fused ? r.part() : nullptr)) return rc;
  return bn_prepare(r, i, y, fused);
}

// BatchNorm backward of conv i:  dx = BN'(xraw; dy masked by the ReLU behind this BatchNorm).  Which mask, and what else is
// read or written, is said by name:
struct BnBwd {
  bool own_relu = false;         // the output went straight through a ReLU (a block's first BN): the mask is rebuilt from xraw with
                                 // the forward's saved scale / shift (ymask and qmask are not read)
  const float* ymask = nullptr;  // else: the post-ReLU activation whose sign is the mask (null: none, the stem's pool backward applied it)
  const unsigned char* qmask = nullptr;   // ymask as one byte per quad, written by bn_act.  The apply kernel reads it instead of ymask
                                 // (32.5 -> 28.2 us); the column reduction keeps the float activation -- with byte loads it got 9 % SLOWER
  bool out16 = false;            // the bf16 data path: dx is stored as bf16, and qmask serves BOTH passes (the activation is bf16 there)
  float* gout = nullptr;         // also write the masked dy here (a block's identity branch)
  int reduced_chunks = 0;        // > 0: the producer of dy left the column sums in the partial-sum buffer, in that many chunks
};
static int bn_backward(const Run& r, int i, const float* xraw, const float* dy, float* dx, const BnBwd& o) {
  const int C = r.p.geom[i].Co;
  const long M = r.rows(i);
  StatCtx sc = stat_ctx(M, C);
  const BnSlots bn = r.bn(i);
  const float* msc = o.own_relu ? bn.scale : NOF;
  const float* msh = o.own_relu ? bn.shift : NOF;
  const float* ymask = o.own_relu ? NOF : o.ymask;
  const bool qred = o.out16 && o.qmask != nullptr;
  if (o.reduced_chunks > 0)
    sc.nchunk = o.reduced_chunks;
  else
    hipLaunchKernelGGL(col_reduce<1>, dim3(sc.nchunk), dim3(256), 0, r.s, xraw, dy, qred ? NOF : ymask,
                       bn.mean, bn.invstd, M, C, sc.rows_per_chunk, r.part(), msc, msh, qred ? o.qmask : (const unsigned char*)nullptr);
  hipLaunchKernelGGL(bn_bwd_finalize, dim3(cdiv(C, FIN_CH)), dim3(256), 0, r.s, r.part(), sc.nchunk, M, C, r.prm->bn_w[i],
                     bn.invstd, r.d->training, r.g->bn_w[i], r.g->bn_b[i], r.at(r.p.coef));
  const long nq = M * C / 4;
  auto apply = o.out16 ? bn_bwd_apply<true> : bn_bwd_apply<false>;
  hipLaunchKernelGGL(apply, dim3(ew_grid(nq)), dim3(256), 0, r.s, xraw, dy, o.qmask ? NOF : ymask,
                     bn.mean, bn.invstd, r.at(r.p.coef), dx, o.gout, nq, C, msc, msh, o.qmask);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

// the part PackTab and UnpackTab share: every convolution's shape and its first workgroup (one per 32 x 32 channel tile; the
// stem's elements go 256 to a workgroup: stem_blocks).  -> the grid
template <class Tab>
static int tab_shapes(Tab& tab, const Plan& p, int stem_blocks) {
  int nb = 0;
  for (int i = 0; i < NCONV; ++i) {
    const Geom& g = p.geom[i];
    tab.cout[i] = g.Co; tab.cin[i] = g.C; tab.ks[i] = g.KS; tab.blk0[i] = nb;
    nb += i == 0 ? stem_blocks : (g.Co / 32) * (g.C / 32);
  }
  tab.blk0[NCONV] = nb; return nb;
}

}  // namespace

// ====================================================================== C ABI
// ---- single-convolution entry points (NHWC activations, packed weights): the building blocks of the trunk,
// exported for unit tests and for bench.py's per-launch roofline timing.
static bool conv_geom(const avvad_conv_desc* d, Geom* g) {
  if (!d || d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->Co <= 0 || d->KS <= 0 || d->stride <= 0 || d->pad < 0)
    return false;
  if (d->H + 2 * d->pad < d->KS || d->W + 2 * d->pad < d->KS) return false;      // (C division rounds -1 / 2 to 0: no window fits)
  const int Ho = (d->H + 2 * d->pad - d->KS) / d->stride + 1, Wo = (d->W + 2 * d->pad - d->KS) / d->stride + 1;
  if (Ho <= 0 || Wo <= 0 || (d->stride != 1 && d->stride != 2)) return false;
  *g = Geom{d->N, d->H, d->W, d->C, Ho, Wo, d->Co, d->KS, d->stride, d->pad};
  return true;
}
extern "C" int avvad_conv2d_pack_weights(const float* w_oihw, float* wf, float* wd, const avvad_conv_desc* d,
                                         avvad_stream_t s) {
  AVVAD_ENTER();
  Geom g;
  if (!w_oihw || !wf || !conv_geom(d, &g)) return AVVAD_EINVAL;
  hipLaunchKernelGGL(pack_weights, dim3(ew_grid((long)g.Co * g.C * g.KS * g.KS)), dim3(256), 0, (hipStream_t)s, w_oihw, wf, wd,
                     g.Co, g.C, g.KS);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
static float* slab_of(void* ws, size_t ws_bytes) { return (ws && ws_bytes >= igemm::SLAB_FLOATS * sizeof(float)) ? (float*)ws : nullptr; }
extern "C" size_t avvad_engine_workspace(void) { return igemm::SLAB_FLOATS * sizeof(float); }
// (one body per direction; the _bf16 entry points below pass b16 = true)
static int conv2d_fwd(bool b16, const void* x, const void* wf, float* y, const avvad_conv_desc* d, void* ws, size_t ws_bytes, avvad_stream_t s) {
  AVVAD_ENTER();
  Geom g;
  if (!x || !wf || !y || !conv_geom(d, &g) || ws_misaligned(ws)) return AVVAD_EINVAL;
  return conv_fwd(b16, (const float*)x, (const float*)wf, y, g, (hipStream_t)s, slab_of(ws, ws_bytes));
}
static int conv2d_dgrad(bool b16, const void* dy, const void* wd, float* dx, const avvad_conv_desc* d, int accumulate, void* ws,
                        size_t ws_bytes, avvad_stream_t s) {
  AVVAD_ENTER();
  Geom g;
  if (!dy || !wd || !dx || !conv_geom(d, &g) || ws_misaligned(ws)) return AVVAD_EINVAL;
  return conv_dgrad(b16, (const float*)dy, (const float*)wd, dx, g, accumulate, (hipStream_t)s, slab_of(ws, ws_bytes));
}
static int conv2d_wgrad(bool b16, const void* x, const void* dy, float* dw_packed, const avvad_conv_desc* d, void* ws, size_t ws_bytes,
                        avvad_stream_t s) {
  AVVAD_ENTER();
  Geom g;
  if (!x || !dy || !dw_packed || !conv_geom(d, &g) || ws_misaligned(ws)) return AVVAD_EINVAL;
  return conv_wgrad(b16, (const float*)x, (const float*)dy, dw_packed, g, (hipStream_t)s, slab_of(ws, ws_bytes));
}
extern "C" int avvad_conv2d_fwd(const float* x, const float* wf, float* y, const avvad_conv_desc* d, void* ws, size_t ws_bytes,
                                avvad_stream_t s) {
  return conv2d_fwd(false, x, wf, y, d, ws, ws_bytes, s);
}
#ifdef AVVAD_PROF
extern "C" int avvad_debug_prof(unsigned long long* out, int reset) {
  if (out) hipMemcpyFromSymbol(out, HIP_SYMBOL(igemm::g_prof), sizeof(unsigned long long) * 8);
  if (reset) { unsigned long long z[8] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(igemm::g_prof), z, sizeof(z)); }
  return 0;
}
extern "C" int avvad_debug_prof_blocks(unsigned long long* out, int n) {
  hipMemcpyFromSymbol(out, HIP_SYMBOL(igemm::g_prof_blk), sizeof(unsigned long long) * 2 * n);
  return 0;
}
extern "C" int avvad_debug_prof_clk(unsigned long long* out, int n) {
  hipMemcpyFromSymbol(out, HIP_SYMBOL(igemm::g_prof_clk), sizeof(unsigned long long) * n);
  return 0;
}
extern "C" int avvad_debug_prof_hw(unsigned long long* out, int n) {
  hipMemcpyFromSymbol(out, HIP_SYMBOL(igemm::g_prof_hw), sizeof(unsigned long long) * n);
  return 0;
}
#endif
extern "C" int avvad_conv2d_dgrad(const float* dy, const float* wd, float* dx, const avvad_conv_desc* d, int accumulate,
                                  void* ws, size_t ws_bytes, avvad_stream_t s) {
  return conv2d_dgrad(false, dy, wd, dx, d, accumulate, ws, ws_bytes, s);
}
extern "C" int avvad_conv2d_wgrad(const float* x, const float* dy, float* dw_packed, const avvad_conv_desc* d, void* ws,
                                  size_t ws_bytes, avvad_stream_t s) {
  return conv2d_wgrad(false, x, dy, dw_packed, d, ws, ws_bytes, s);
}

// ---- the bf16 data path's convolutions on their own (bgemm.h): operands bf16 in HBM, fp32 results.  Exported for the
// parity tests and bench.py's bf16 roofline probe; the trunk calls the same launchers when option "bf16" is 1.
namespace {
__global__ void pack_weights_bf16(const float* __restrict__ w, __bf16* __restrict__ wf16, __bf16* __restrict__ wd16, int Co, int C, int KS) {
  const int T = KS * KS, n = Co * C * T;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int r = i;                                                 // i indexes OIHW
    const int tap = r % T; r /= T;
    const int c = r % C; const int co = r / C;
    const __bf16 v = (__bf16)w[i];
    wf16[(long)co * (T * C) + ((c >> 6) * T + tap) * 64 + (c & 63)] = v;
    if (wd16) wd16[(long)c * (T * Co) + ((co >> 6) * T + tap) * 64 + (co & 63)] = v;
  }
}
}  // namespace
extern "C" int avvad_conv2d_pack_weights_bf16(const float* w_oihw, void* wf16, void* wd16, const avvad_conv_desc* d, avvad_stream_t s) {
  AVVAD_ENTER();
  Geom g;
  if (!w_oihw || !wf16 || !conv_geom(d, &g) || g.C % 64 || g.Co % 64) return AVVAD_EINVAL;
  hipLaunchKernelGGL(pack_weights_bf16, dim3(ew_grid((long)g.Co * g.C * g.KS * g.KS)), dim3(256), 0, (hipStream_t)s, w_oihw,
                     (__bf16*)wf16, (__bf16*)wd16, g.Co, g.C, g.KS);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
extern "C" int avvad_conv2d_fwd_bf16(const void* x16, const void* wf16, float* y, const avvad_conv_desc* d, void* ws, size_t ws_bytes,
                                     avvad_stream_t s) {
  return conv2d_fwd(true, x16, wf16, y, d, ws, ws_bytes, s);
}
extern "C" int avvad_conv2d_dgrad_bf16(const void* dy16, const void* wd16, float* dx, const avvad_conv_desc* d, int accumulate,
                                       void* ws, size_t ws_bytes, avvad_stream_t s) {
  return conv2d_dgrad(true, dy16, wd16, dx, d, accumulate, ws, ws_bytes, s);
}
extern "C" int avvad_conv2d_wgrad_bf16(const void* x16, const void* dy16, float* dw_packed, const avvad_conv_desc* d, void* ws,
                                       size_t ws_bytes, avvad_stream_t s) {
  return conv2d_wgrad(true, x16, dy16, dw_packed, d, ws, ws_bytes, s);
}

extern "C" size_t avvad_trunk_workspace(const avvad_trunk_desc* d) {
  if (!trunk_desc_ok(d)) return 0;
  const Plan p = make_plan(d);
  return p.total * sizeof(float);
}

// Where the post-ReLU activations a forward run with save_for_backward keeps in its workspace live (test support: the
// parity tests compare their sign patterns with the oracle's to tell a flipped ReLU unit from an indexing error).
// index 0: pooled stem output; 1 + 2k: block k's first activation (after bn1 + ReLU); 2 + 2k: block k's output. NHWC.
// the last index, 17: the pool's arg-max plane (N * H * W * 16 32-bit words, byte k of word q: window position dh*3+dw of channel 4q+k).
extern "C" int avvad_trunk_activation(const avvad_trunk_desc* d, int index, size_t* offset_floats, int* C, int* H, int* W) {
  constexpr int ARGMAX = 1 + 2 * NBLOCK;
  if (!trunk_desc_ok(d) || index < 0 || index > ARGMAX || !offset_floats || !C || !H || !W) return AVVAD_EINVAL;
  if (index == ARGMAX && !d->save_for_backward) return AVVAD_EINVAL;     // (the plane is written only for a backward)
  const Plan p = make_plan(d);
  if (index == 0 || index == ARGMAX) {
    *offset_floats = index == 0 ? p.p0 : p.am; *C = 64; *H = p.h[2]; *W = p.w[2];
    return AVVAD_OK;
  }
  const Block& k = p.block[(index - 1) / 2];
  *offset_floats = (index - 1) % 2 == 0 ? k.a1 : k.out;
  *C = k.width; *H = k.h; *W = k.w;
  return AVVAD_OK;
}

extern "C" int avvad_trunk_fwd(const float* frames, const avvad_trunk_params* prm, float* feat, const avvad_trunk_desc* d,
                               void* wsv, size_t ws_bytes, avvad_stream_t sv) {
  AVVAD_ENTER();
  if (!frames || !prm || !feat || !wsv || ws_misaligned(wsv) || !trunk_desc_ok(d)) return AVVAD_EINVAL;
  const Plan p = make_plan(d);
  if (ws_bytes < p.total * sizeof(float)) return AVVAD_EWORKSPACE;
  const Run r{p, (float*)wsv, prm, nullptr, d, (hipStream_t)sv};
  hipStream_t s = r.s; int rc;
  const bool b16 = native_bf16();        // the bf16 data path: activations between convolutions are stored as bf16
  const bool save = d->save_for_backward;
  // weights: OIHW -> packed
  PackTab tab;
  const int nb = tab_shapes(tab, p, cdiv(64 * 49, 256));
  for (int i = 0; i < NCONV; ++i) {
    tab.w[i] = prm->conv_w[i];
    tab.wf[i] = r.at(p.wf[i]);
    tab.wd[i] = (i > 0 && save) ? r.at(p.wd[i]) : nullptr;
    tab.wf16[i] = (b16 && i > 0) ? reinterpret_cast<__bf16*>(r.at(p.wf16[i])) : nullptr;
    tab.wd16[i] = (b16 && i > 0 && save) ? reinterpret_cast<__bf16*>(r.at(p.wd16[i])) : nullptr;
  }
  hipLaunchKernelGGL(pack_all, dim3(nb), dim3(256), 0, s, tab);
  // stem
  if ((rc = conv_bn(r, 0, frames, r.at(p.c0)))) return rc;
  const BnSlots bn0 = r.bn(0);
  unsigned* am = save ? reinterpret_cast<unsigned*>(r.at(p.am)) : nullptr;
  auto pool = b16 ? stem_bn_relu_pool<true> : stem_bn_relu_pool<false>;
  hipLaunchKernelGGL(pool, dim3(ew_grid((long)d->N * p.h[2] * p.w[2] * 16)), dim3(256), 0, s, r.at(p.c0), bn0.scale, bn0.shift, r.at(p.p0), am,
                     d->N, p.h[1], p.w[1], p.h[2], p.w[2]);
  // residual stages (bn_act writes bf16 on the bf16 data path; the residual it adds is bf16 there only when it is the block's input)
  auto act = b16 ? bn_act<true, false> : bn_act<false, false>;
  auto act_id = b16 ? bn_act<true, true> : bn_act<false, false>;
  for (const Block& k : p.block) {
    const int C = k.width;
    const long nq = k.M * C / 4;
    const float* x = r.at(k.in);
    unsigned char* qmo = save ? reinterpret_cast<unsigned char*>(r.at(k.qm)) : nullptr;
    const BnSlots bn1 = r.bn(k.i1), bn2 = r.bn(k.i2);
    if ((rc = conv_bn(r, k.i1, x, r.at(k.c1)))) return rc;
    hipLaunchKernelGGL(act, dim3(ew_grid(nq)), dim3(256), 0, s, r.at(k.c1), bn1.scale, bn1.shift, NOF, NOF, NOF, r.at(k.a1), nq, C, 1,
                       (unsigned char*)nullptr);
    if ((rc = conv_bn(r, k.i2, r.at(k.a1), r.at(k.c2)))) return rc;
    if (k.ds) {
      if ((rc = conv_bn(r, k.id, x, r.at(k.cd)))) return rc;
      const BnSlots bnd = r.bn(k.id);
      // (the identity input is the downsample convolution's RAW fp32 output in either data path)
      hipLaunchKernelGGL(act, dim3(ew_grid(nq)), dim3(256), 0, s, r.at(k.c2), bn2.scale, bn2.shift, r.at(k.cd), bnd.scale, bnd.shift,
                         r.at(k.out), nq, C, 1, qmo);
    } else {
      hipLaunchKernelGGL(act_id, dim3(ew_grid(nq)), dim3(256), 0, s, r.at(k.c2), bn2.scale, bn2.shift, x, NOF, NOF, r.at(k.out), nq, C, 1, qmo);
    }
  }
  const Block& last = p.block[NBLOCK - 1];
  auto avg = b16 ? avgpool_fwd<true> : avgpool_fwd<false>;
  hipLaunchKernelGGL(avg, dim3(ew_grid((long)d->N * last.width)), dim3(256), 0, s, r.at(last.out), feat, d->N, last.h * last.w, last.width);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}

extern "C" int avvad_trunk_bwd(const float* frames, const avvad_trunk_params* prm, const float* dfeat,
                               const avvad_trunk_grads* g, const avvad_trunk_desc* d, void* wsv, size_t ws_bytes,
                               avvad_stream_t sv) {
  AVVAD_ENTER();
  BwdCuCap cu_cap;
  if (!frames || !prm || !dfeat || !g || !wsv || ws_misaligned(wsv) || !trunk_desc_ok(d) || !d->save_for_backward) return AVVAD_EINVAL;
  const Plan p = make_plan(d);
  if (ws_bytes < p.total * sizeof(float)) return AVVAD_EWORKSPACE;
  const Run r{p, (float*)wsv, prm, g, d, (hipStream_t)sv};
  hipStream_t s = r.s; int rc;
  float *G0 = r.at(p.G[0]), *G1 = r.at(p.G[1]), *G2 = r.at(p.G[2]), *G3 = r.at(p.G[3]);
  // d(out of last block) from the average pool
  const Block& last = p.block[NBLOCK - 1];
  hipLaunchKernelGGL(avgpool_bwd, dim3(ew_grid(last.M * last.width)), dim3(256), 0, s, dfeat, G0, d->N, last.h * last.w, last.width);
  const bool b16 = native_bf16();        // the forward ran the bf16 data path (same process-wide option): activations,
                                         // and the BatchNorm-backward outputs that feed convolutions, are bf16
  const size_t* wd = b16 ? p.wd16 : p.wd;      // the data path's data-gradient packs
  // (weight gradients: wanted ones only, into p.wg[i], unpacked at the end by unpack_all)
  // (the stem's is fp32 on either data path)
  auto wgrad = [&](int i, const float* x, const float* dy) {
    return g->conv_w[i] ? conv_wgrad(i > 0 && b16, x, dy, r.at(p.wg[i]), p.geom[i], s, r.at(p.slab)) : AVVAD_OK;
  };
  auto dgrad = [&](int i, const float* dy, float* dx, int acc) { return conv_dgrad(b16, dy, r.at(wd[i]), dx, p.geom[i], acc, s, r.at(p.slab)); };
  for (int kb = NBLOCK - 1; kb >= 0; --kb) {
    const Block& k = p.block[kb];
    const float* x = r.at(k.in);
    // G0 = d(block output, post-ReLU).  BN2 and the downsample's BN sit under the block output's ReLU; BN1 under its own
    BnBwd under_out, under_own;
    under_out.ymask = r.at(k.out);
    under_out.qmask = reinterpret_cast<const unsigned char*>(r.at(k.qm));
    under_out.out16 = under_own.out16 = b16; under_own.own_relu = true;
    if (k.ds) {
      if ((rc = bn_backward(r, k.i2, r.at(k.c2), G0, G1, under_out))) return rc;           // main branch: d c2 in G1
      if ((rc = bn_backward(r, k.id, r.at(k.cd), G0, G2, under_out))) return rc;           // identity branch, downsample BN: d cd in G2
      if ((rc = wgrad(k.id, x, G2))) return rc;
      if ((rc = dgrad(k.id, G2, G3, 0))) return rc;                                        // ... and its 1x1 conv: d x in G3
    } else {
      under_out.gout = G3;                                                                 // identity branch: d x = masked d out
      if ((rc = bn_backward(r, k.i2, r.at(k.c2), G0, G1, under_out))) return rc;           // main branch: d c2 in G1
    }
    if ((rc = wgrad(k.i2, r.at(k.a1), G1))) return rc;
    if ((rc = dgrad(k.i2, G1, G2, 0))) return rc;                                        // d a1 in G2
    if ((rc = bn_backward(r, k.i1, r.at(k.c1), G2, G1, under_own))) return rc;           // d c1 in G1
    if ((rc = wgrad(k.i1, x, G1))) return rc;
    if ((rc = dgrad(k.i1, G1, G3, 1))) return rc;                                        // d x += ...
    float* t = G0; G0 = G3; G3 = t;
  }
  // stem: G0 = d p0
  if (g->conv_w[0] || g->bn_w[0] || g->bn_b[0]) {
    float* g0 = r.at(p.g0);
    const BnSlots bn0 = r.bn(0);
    // the BatchNorm backward's column sums (sum g0, sum g0 xhat) are formed here, where g0 is produced: 2048 workgroups = chunks
    const bool fuse0 = !avvad_tune().no_fused_stats;
    int grid0 = ew_grid((long)d->N * p.h[1] * p.w[1] * 16);
    if (fuse0 && grid0 > 2048) grid0 = 2048;
    hipLaunchKernelGGL(stem_pool_relu_bwd, dim3(grid0), dim3(256), 0, s, r.at(p.c0), bn0.scale, bn0.shift,
                       reinterpret_cast<const unsigned*>(r.at(p.am)), G0, g0, d->N, p.h[1], p.w[1], p.h[2], p.w[2],
                       fuse0 ? bn0.mean : NOF, fuse0 ? bn0.invstd : NOF, fuse0 ? r.part() : (double*)nullptr);
    // in place: d c0 overwrites g0.  No mask: the pool's backward applied the stem's ReLU
    BnBwd stem; stem.reduced_chunks = fuse0 ? grid0 : 0;
    if ((rc = bn_backward(r, 0, r.at(p.c0), g0, g0, stem))) return rc;
    if ((rc = wgrad(0, frames, g0))) return rc;
  }
  UnpackTab tab;
  const int nb = tab_shapes(tab, p, cdiv(64 * 3 * 49, 256));
  bool any = false;
  for (int i = 0; i < NCONV; ++i) {
    tab.pk[i] = r.at(p.wg[i]);
    tab.dw[i] = g->conv_w[i];      // null: not wanted
    any = any || g->conv_w[i];
  }
  if (any) hipLaunchKernelGGL(unpack_all, dim3(nb), dim3(256), 0, s, tab);
  AVVAD_LAUNCH_CHECK();
  return AVVAD_OK;
}
