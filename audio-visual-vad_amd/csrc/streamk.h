// streamk.h -- the stream-K schedule that the two GEMM engines share (igemm.h: fp32 operands; bgemm.h: operands bf16 in
// memory): the share arithmetic, the fix-up kernels that combine split tiles, and the host's launch plan.  The engines' kernels
// walk their shares and store their tiles themselves (the same text in both), but every share
// bound they use comes from Share below -- the type the fix-up kernels invert.
//
// Work decomposition: data-parallel rounds + one "stream-K" round.  The launch creates G persistent workgroups
// (= the number resident at once: 256 CUs x workgroups/CU).  Worker g first takes whole tiles g, g+G, ... for
// `full_rounds` rounds (plain stores, all workers walk K in step -> weight panels are shared in L2); the
// remaining rem_tiles < G tiles are then treated as ONE pool of R = rem_tiles x ktiles BK-deep iterations cut into G
// equal contiguous shares (Share below): a tile may be split between workers.  The worker whose share STARTS a tile's K
// range stores its piece onto the output, the others leave theirs in their slabs (one tile-sized slot per worker), and a
// fix-up kernel adds a tile's slabs onto its output in ascending worker (= ascending K) order: no atomics, no pre-zeroed
// output, bit-reproducible.  That removes the tile-quantisation loss of e.g. 648 or 288 tiles on 512 resident slots
// (37 % / 44 % idle).  (Only the K-major tuning mode of igemm::kernel, off by default, adds atomically.)
// Measured balance of this static split (tools/lab/prof_conv.py, -DAVVAD_PROF): all G workers start within 0.5 us; the
// two workgroups of a CU are raw block ids b and b+256 and the OLDER always finishes first (192 vs 237 us: the matrix
// pipe is arbitrated oldest-first); XCDs finish up to 17 % apart on equal shares (the same two are slowest for every
// shape on a given device).  Tried and dropped: age-skewed shares (+-1 %), a dynamically pulled tail pool of 8-K-tile
// pieces (1-5 % slower: every piece pays a prologue and a 64 KB atomic flush), K-major cells for the weight gradients
// (less HBM traffic, 2 % slower end to end), staggering the co-residents' phases (no effect), requesting the NEXT
// segment's first K tile before the epilogue (the prefetched registers live across the epilogue: past the 128-VGPR
// budget of 4 waves/SIMD the 8-wave kernels spill, 5 % slower end to end).
#pragma once
#include "common.h"
#include <type_traits>

namespace igemm {

// ---------------------------------------------------------------- what an epilogue may carry (detected by member)
template <class Epi, class = void>
struct HasStat : std::false_type {};      // `stat`: fused column statistics (EpiStore::stat)
template <class Epi>
struct HasStat<Epi, std::void_t<decltype(Epi::stat)>> : std::true_type {};
template <class Epi, class = void>
struct HasSched : std::false_type {};     // `sched`: tiles of different lengths, all of them in the pool (ClassSched, TapSched)
template <class Epi>
struct HasSched<Epi, std::void_t<decltype(Epi::sched)>> : std::true_type {};
// epilogues whose output is a plain row-major matrix (C, ldc, cs, mode) take the fast store path
template <class Epi, class = void>
struct IsPlain : std::false_type {};
template <class Epi>
struct IsPlain<Epi, std::void_t<decltype(Epi::PLAIN)>> : std::integral_constant<bool, Epi::PLAIN> {};
// An epilogue may FINISH elements: `finish4(m, n0, v, N)` receives the final sums of up to four consecutive columns of row m
// from the fix-up kernel (the one place where a split tile's total exists) and does whatever follows the product -- the
// LSTM backward runs the previous step's gate arithmetic there, one launch less per time step.  It is only honoured when
// EVERY tile of the product passes through the stream-K pool (launch() tells the caller through `finished`); `active` is
// set by launch().
template <class Epi, class = void>
struct HasFinish : std::false_type {};
template <class Epi>
struct HasFinish<Epi, std::void_t<decltype(&Epi::finish4)>> : std::true_type {};
template <class Epi>
__device__ __forceinline__ bool epi_live(const Epi& E, int m, int M) {
  if constexpr (HasSched<Epi>::value) return m < M && E.live(m);
  else return m < M;
}

// ---------------------------------------------------------------- share arithmetic
// The pool's R iterations are cut into G shares: worker g owns [g*R/G, (g+1)*R/G), so iteration `it` belongs to worker
// ceil((it+1)*G/R) - 1.  The kernels' walk (forward) and the fix-up kernels (inverse: which workers cut a tile) must agree
// exactly -- a fix-up that expects a slab nobody wrote adds garbage -- so both use this type and nothing else.
// T = long in the kernels.  T = unsigned in the fix-up kernels, where all of this is block-uniform and in 32 bits (the host
// launches them only when R * G < 4e9, see fits32(): a 64-bit software division per thread and slab was most of the
// fix-up's time in its first version).
template <class T>
struct Share {
  T R, G;
  template <class Epi>
  __host__ __device__ __forceinline__ static Share of(const Epi& E, int rem_tiles, int ktiles, T G) {
    if constexpr (HasSched<Epi>::value) return Share{(T)E.sched.total(), G};
    else return Share{(T)rem_tiles * (T)ktiles, G};
  }
  __host__ __device__ __forceinline__ T lo(T g) const { return g * R / G; }
  __host__ __device__ __forceinline__ T hi(T g) const { return (g + 1) * R / G; }
  // fewer iterations than workers: some shares are empty, and a worker with an empty share wrote no slab.  (The fix-ups test
  // wrote() only when sparse(), hoisted out of their loops: two divisions per slab otherwise.)
  __host__ __device__ __forceinline__ bool sparse() const { return R < G; }
  __host__ __device__ __forceinline__ bool wrote(T g) const { return hi(g) > lo(g); }
  __host__ __device__ __forceinline__ int owner(T it) const { return (int)(((it + 1) * G + R - 1) / R) - 1; }
  // tile tr of the pool <-> iterations [it0, it1]: the tiles' K tiles back to back (uniform: ktiles each)
  template <class Epi>
  __host__ __device__ __forceinline__ void span(const Epi& E, int tr, int ktiles, T& it0, T& it1) const {
    if constexpr (HasSched<Epi>::value) { it0 = (T)E.sched.base(tr); it1 = it0 + (T)E.sched.len(tr) - 1; }
    else { it0 = (T)tr * (T)ktiles; it1 = it0 + (T)ktiles - 1; }
  }
  template <class Epi>
  __device__ __forceinline__ static void locate(const Epi& E, T it, int ktiles, T& tr, int& kt, int& klen) {
    if constexpr (HasSched<Epi>::value) { int tile; E.sched.locate(it, tile, kt, klen); tr = tile; }
    else { tr = it / ktiles; kt = (int)(it - tr * ktiles); klen = ktiles; }
  }
  // first and last worker of tile tr (gb > ga: the tile was split, workers ga+1 .. gb left their pieces in their slabs;
  // shares are contiguous, so every non-empty worker between ga and gb lies inside this tile)
  template <class Epi>
  __host__ __device__ __forceinline__ void cut(const Epi& E, int tr, int ktiles, int& ga, int& gb) const {
    T it0, it1;
    span(E, tr, ktiles, it0, it1);
    ga = owner(it0);
    gb = owner(it1);
  }
};

// ---------------------------------------------------------------- the fix-up kernels
// Fix-up of the stream-K round: tile tr of the remainder pool was cut between workers ga .. gb (ascending K).  Worker ga
// stored (or accumulated) its piece onto the output, workers ga+1 .. gb left theirs in their slabs; this kernel adds those
// slabs in a FIXED order -- so the result is bit-reproducible run to run.  It replaces both the zero-fill launch in front
// of the GEMM and the float atomics inside it.
// One workgroup = 4 waves per 256-element strip of a tile (lane = one float4): wave w sums the tile's slabs ga+1+w,
// ga+1+w+4, ... with four loads in flight, the four partial sums meet in LDS in wave order.  (First version: one thread
// walked all of a tile's slabs in a serial loop -- latency-bound, 37 us for the 31-way split tiles of the LSTM's
// recurrent products.)
template <int BM, int BN, class Epi>
__global__ void __launch_bounds__(256)
    fixup(const Epi E, const float* __restrict__ slab, const int M, const int N, const int ktiles, const long G,
          const int full_rounds, const int rem_tiles, const int ntn) {
  constexpr int STRIPS = BM * BN / 256;                  // 256-element strips per tile
  __shared__ float4 part[3][64];
  const int tr = blockIdx.x / STRIPS, strip = blockIdx.x % STRIPS;
  const Share<unsigned> sh = Share<unsigned>::of(E, rem_tiles, ktiles, (unsigned)G);
  int ga, gb;
  sh.cut(E, tr, ktiles, ga, gb);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e0 = strip * 256 + lane * 4;                 // tile-local element (row-major [BM][BN]) of this lane's float4
  if (gb <= ga) {                                        // the tile was not split: its output is final already
    if constexpr (HasFinish<Epi>::value) {
      if (E.active && wave == 0) {
        const unsigned tile_u = (unsigned)full_rounds * sh.G + (unsigned)tr;
        const int mu = (int)(tile_u / (unsigned)ntn) * BM + e0 / BN, nu = (int)(tile_u % (unsigned)ntn) * BN + e0 % BN;
        if (epi_live(E, mu, M)) {
          float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (nu + e < N) v[e] = *E.ptr(mu, nu + e);
          E.finish4(mu, nu, v, N);
        }
      }
    }
    return;
  }
  const bool sparse = sh.sparse();
  const float* S0 = slab + e0;
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int g = ga + 1 + wave; g <= gb; g += 16) {
    float4 v[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int gu = g + 4 * u;
      ok[u] = gu <= gb && (!sparse || sh.wrote((unsigned)gu));       // (an empty share's slot holds nothing: skipped)
      v[u] = *reinterpret_cast<const float4*>(S0 + (long)(ok[u] ? gu : ga + 1) * (BM * BN));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (ok[u]) { sum.x += v[u].x; sum.y += v[u].y; sum.z += v[u].z; sum.w += v[u].w; }
  }
  if (wave > 0) part[wave - 1][lane] = sum;
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int w = 0; w < 3; ++w) { const float4 p = part[w][lane]; sum.x += p.x; sum.y += p.y; sum.z += p.z; sum.w += p.w; }
  const unsigned tile = (unsigned)full_rounds * sh.G + (unsigned)tr;
  const int m = (int)(tile / (unsigned)ntn) * BM + e0 / BN, n0 = (int)(tile % (unsigned)ntn) * BN + e0 % BN;
  if (!epi_live(E, m, M)) return;
  const float sv[4] = {sum.x, sum.y, sum.z, sum.w};
  if constexpr (HasFinish<Epi>::value) {
    if (E.active) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n0 + e < N) v[e] = *E.ptr(m, n0 + e) + sv[e];
      E.finish4(m, n0, v, N);
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (n0 + e < N) *E.ptr(m, n0 + e) += sv[e];
}

// The same fix-up for SHALLOW splits (a tile cut between a handful of workers: the convolutions' stream-K rounds): one WAVE
// per strip, four strips per workgroup, the wave walks its tile's slabs itself.  The kernel above spends four waves, an LDS
// exchange and a barrier on every strip; with ~3 slabs per tile three of them load one slab each -- a 136-tile round was
// 34816 waves for 43 MB, 15 us.  (Deep splits -- the LSTM's 31-way, the weight gradients' 100-way tiles -- keep the
// four-wave form.)
template <int BM, int BN, class Epi>
__global__ void __launch_bounds__(256)
    fixup1(const Epi E, const float* __restrict__ slab, const int M, const int N, const int ktiles, const long G,
           const int full_rounds, const int rem_tiles, const int ntn) {
  constexpr int STRIPS = BM * BN / 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sg = blockIdx.x * 4 + wave;
  const int tr = sg / STRIPS, strip = sg % STRIPS;
  if (tr >= rem_tiles) return;
  const Share<unsigned> sh = Share<unsigned>::of(E, rem_tiles, ktiles, (unsigned)G);
  int ga, gb;
  sh.cut(E, tr, ktiles, ga, gb);
  const int e0 = strip * 256 + lane * 4;
  const unsigned tile = (unsigned)full_rounds * sh.G + (unsigned)tr;
  const int m = (int)(tile / (unsigned)ntn) * BM + e0 / BN, n0 = (int)(tile % (unsigned)ntn) * BN + e0 % BN;
  if (!epi_live(E, m, M)) return;
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  if (gb > ga) {
    const bool sparse = sh.sparse();
    const float* S0 = slab + e0;
    for (int g = ga + 1; g <= gb; g += 4) {
      float4 v[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int gu = g + u;
        ok[u] = gu <= gb && (!sparse || sh.wrote((unsigned)gu));
        v[u] = *reinterpret_cast<const float4*>(S0 + (long)(ok[u] ? gu : ga + 1) * (BM * BN));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ok[u]) { sum.x += v[u].x; sum.y += v[u].y; sum.z += v[u].z; sum.w += v[u].w; }
    }
  } else if (!HasFinish<Epi>::value) {
    return;                                              // unsplit tile, nothing to finish
  }
  const float sv[4] = {sum.x, sum.y, sum.z, sum.w};
  if constexpr (HasFinish<Epi>::value) {
    if (E.active) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n0 + e < N) v[e] = *E.ptr(m, n0 + e) + sv[e];
      E.finish4(m, n0, v, N);
      return;
    }
    if (gb <= ga) return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (n0 + e < N) *E.ptr(m, n0 + e) += sv[e];
}

// Fix-up of split tiles WITH the fused column statistics (EpiStore::stat): one workgroup per remainder tile.  Thread
// (cq, rg) owns the float4 column cq of rows rg, rg + RG, ...: it adds the tile's slabs in ascending worker order onto the
// piece the first worker stored, writes the total back and keeps sum / sum of squares of its columns (fp32 over its BM / RG
// rows, then doubles); the RG row groups meet in LDS in a fixed order.  Tiles that one worker finished by itself are skipped
// (the kernel wrote their statistics).
template <int BM, int BN, class Epi>
__global__ void __launch_bounds__(256)
    fixup_tile(const Epi E, const float* __restrict__ slab, const int M, const int N, const int ktiles, const long G,
               const int full_rounds, const int rem_tiles, const int ntn) {
  constexpr int CQ = BN / 4, RG = 256 / CQ, RPT = BM / RG;
  static_assert(RPT % 4 == 0, "four rows in flight per thread");
  __shared__ double red[RG * BN * 2];
  const int tr = blockIdx.x;
  const Share<unsigned> sh = Share<unsigned>::of(E, rem_tiles, ktiles, (unsigned)G);
  int ga, gb;
  sh.cut(E, tr, ktiles, ga, gb);
  if (gb <= ga) return;                                  // block-uniform
  const bool sparse = sh.sparse();
  const unsigned tile = (unsigned)full_rounds * sh.G + (unsigned)tr;
  const int tm = (int)(tile / (unsigned)ntn);
  const int m0 = tm * BM, n0 = (int)(tile % (unsigned)ntn) * BN;
  float* Cv = E.C;
  int mrow0 = m0, Mv = M;
  if constexpr (HasSched<Epi>::value) { const auto v = E.view(m0); Cv = v.C; mrow0 = v.row0; Mv = v.M; }
  const int cq = threadIdx.x % CQ, rg = threadIdx.x / CQ;
  const int n = n0 + cq * 4;
  float s4[4] = {0.f, 0.f, 0.f, 0.f}, q4[4] = {0.f, 0.f, 0.f, 0.f};
  if (n < N) {                                           // (N % 4 == 0: a float4 column is inside or outside as a whole)
#pragma unroll 1
    for (int rr = 0; rr < RPT; rr += 4) {
      float4 tot[4];
      bool live[4];
      const float* sp[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = rg + RG * (rr + u);
        live[u] = mrow0 + row < Mv;
        sp[u] = slab + (long)(live[u] ? row : 0) * BN + cq * 4;
        tot[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      for (int g = ga + 1; g <= gb; ++g) {
        if (sparse && !sh.wrote((unsigned)g)) continue;  // this worker's share was empty
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(sp[u] + (long)g * (BM * BN));
#pragma unroll
        for (int u = 0; u < 4; ++u) { tot[u].x += v[u].x; tot[u].y += v[u].y; tot[u].z += v[u].z; tot[u].w += v[u].w; }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!live[u]) continue;
        float4* const cp = reinterpret_cast<float4*>(Cv + (long)(mrow0 + rg + RG * (rr + u)) * E.ldc + n);
        float4 o = *cp;
        o.x += tot[u].x; o.y += tot[u].y; o.z += tot[u].z; o.w += tot[u].w;
        *cp = o;
        s4[0] += o.x; s4[1] += o.y; s4[2] += o.z; s4[3] += o.w;
        q4[0] = fmaf(o.x, o.x, q4[0]); q4[1] = fmaf(o.y, o.y, q4[1]); q4[2] = fmaf(o.z, o.z, q4[2]); q4[3] = fmaf(o.w, o.w, q4[3]);
      }
    }
  }
  if (E.stat == nullptr) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[(rg * BN + cq * 4 + e) * 2 + 0] = (double)s4[e];
    red[(rg * BN + cq * 4 + e) * 2 + 1] = (double)q4[e];
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < BN && n0 + c < N) {
    double a = 0, b = 0;
#pragma unroll 4
    for (int w = 0; w < RG; ++w) { a += red[(w * BN + c) * 2 + 0]; b += red[(w * BN + c) * 2 + 1]; }
    E.stat[((long)tm * 2 + 0) * N + n0 + c] = a;
    E.stat[((long)tm * 2 + 1) * N + n0 + c] = b;
  }
}

// ---------------------------------------------------------------- the host plan
// Floats of slab workspace a launch may need: one BM x BN tile per persistent worker (512 x 128x128 = 1024 x 128x64 =
// 1536 x 64x64 at most).  Callers carve this out of their own workspace (the C ABI's caller-allocates rule).
// (... or one [576][64] weight-gradient partial per CU, conv64.h: 256 x 36864, the larger of the two)
constexpr size_t SLAB_FLOATS = (size_t)256 * 576 * 64;
static_assert(SLAB_FLOATS >= (size_t)512 * 128 * 128, "one 128x128 tile per persistent worker");

// persistent workers of a kernel with per_cu resident workgroups per CU: what is resident at once, within the slab space
static inline long workers(int per_cu, int BM, int BN) {
  long G = (long)grid_cus() * per_cu;
  if (G * BM * BN > (long)SLAB_FLOATS) G = (long)(SLAB_FLOATS / ((size_t)BM * BN));
  return G;
}

// the fix-up kernels' index math (Share<unsigned>) is 32-bit: a pool of R iterations on G workers must keep R * G below 2^32
static inline bool fits32(double R, long G) { return R * (double)G < 4.0e9; }

struct Rounds { long G; int full_rounds, rem; };
// ntiles uniform tiles of ktiles K tiles on G workers -> full rounds + the stream-K pool's tiles.  `slab` null (or the
// "no_streamk" option for this mode) selects whole-tile scheduling.
static inline Rounds plan_rounds(long ntiles, int ktiles, long G, bool slab, int mode) {
  const AvvadTune& tn = avvad_tune();
  const bool no_sk = !slab || tn.no_streamk == 1 || tn.no_streamk == 10 + mode || !fits32((double)ntiles * ktiles, G);
  long full_rounds = ntiles / G, rem = ntiles - full_rounds * G;
  if (no_sk || rem * 10 >= G * 9) {   // (nearly) full last round: keep it data-parallel
    if (rem > 0) ++full_rounds;
    rem = 0;
  }
  if (rem > 0 && full_rounds == 0) {  // fewer tiles than workers: >= 4 iterations per worker amortise prologue/epilogue
    const long iters = ntiles * ktiles, cap = iters / 4 > 0 ? iters / 4 : 1;
    if (G > cap) G = cap;
  }
  return Rounds{G, (int)full_rounds, (int)rem};
}

// what the fused column statistics need of the output (EpiStore::stat; position classes: whole float4s per pixel too)
template <class Epi>
static inline bool stat_ok(const Epi& e, int N, int kchunks = 0) {
  if constexpr (HasStat<Epi>::value) {
    if (e.stat == nullptr) return true;
    if (e.cs != 1 || (e.ldc & 3) || (N & 3) || (((uintptr_t)e.C) & 15) || kchunks > 0 || e.bias != nullptr) return false;
    if constexpr (HasSched<Epi>::value) return (e.W & 3) == 0;
  }
  return true;
}

// the fix-up of a launch whose pool holds rt > 0 tiles.  `deep`: splits of up to this many slabs per tile (a handful: the
// convolutions) take the one-wave-per-strip kernel; 0 = always the four-wave kernel
constexpr int FIXUP1_DEPTH = 6;
template <int BM, int BN, class Epi>
static inline void launch_fixup(const Epi& e, const float* slab, int M, int N, int ktiles, long G, int fr, int rt, hipStream_t s,
                                int deep = FIXUP1_DEPTH) {
  const int ntn = cdiv(N, BN);
  if constexpr (HasStat<Epi>::value) {
    if (e.stat != nullptr) {
      hipLaunchKernelGGL((fixup_tile<BM, BN, Epi>), dim3(rt), dim3(256), 0, s, e, slab, M, N, ktiles, G, fr, rt, ntn);
      return;
    }
  }
  if ((G + rt - 1) / rt <= deep)
    hipLaunchKernelGGL((fixup1<BM, BN, Epi>), dim3(rt * (BM * BN / 1024)), dim3(256), 0, s, e, slab, M, N, ktiles, G, fr, rt, ntn);
  else
    hipLaunchKernelGGL((fixup<BM, BN, Epi>), dim3(rt * (BM * BN / 256)), dim3(256), 0, s, e, slab, M, N, ktiles, G, fr, rt, ntn);
}

// Plan of a position-class product (ClassSched / TapSched: every tile is in the pool, tiles differ in length) on 128x128
// tiles, two workgroups per CU.  Needs the scratch; AVVAD_EINVAL = nothing can be launched, the caller falls back.
template <class Epi>
static inline int plan_cls(const Epi& e, int Mp, int N, const float* slab, long& G, int& ntiles) {
  if (Mp <= 0 || N <= 0 || !slab) return AVVAD_EINVAL;
  ntiles = (int)((long)cdiv(Mp, 128) * cdiv(N, 128));
  G = workers(2, 128, 128);
  const long R = e.sched.total();
  if (R <= 0 || !fits32((double)R, G)) return AVVAD_EINVAL;
  if (G > R / 4) G = R / 4 > 0 ? R / 4 : 1;
  return stat_ok(e, N) ? AVVAD_OK : AVVAD_EINVAL;
}

}  // namespace igemm
