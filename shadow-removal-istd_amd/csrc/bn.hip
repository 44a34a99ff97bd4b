// BatchNorm2d forward statistics / finalize and the fused BN + activation backward
// (STCGAN/networks.py:107,109,170,179; activations :106,108,158,171,180).
//
// Forward: the conv epilogue writes the raw (pre-BN) output; stc_chan_stats
// reduces per-channel shifted sums over pixel chunks, stc_bn_finalize merges
// the chunks in a fixed order (Chan's parallel variance, fp64) and emits the
// (scale, shift) table that the *consumer* GEMM applies as its load prologue,
// plus the running-stat update.  Nothing normalised is written to HBM.
// Backward: dn = g1*act1'(n) + g2*act2'(n) is recomputed on the fly from the raw
// input (n = x*scale + shift), reduced to sum(dn), sum(dn*xhat), then applied.
// On running statistics (eval mode / frozen layers) dx = scale*dn needs no sum: one pass (stc_bn_bwd_frozen).
// Sync statistics (nn.SyncBatchNorm): stc_bn_stats_pack turns a rank's partials into one record
// per channel, stc_bn_finalize over the ranks' records is the global finalize; backward, stc_bn_bwd_sums emits the
// rank's sums as a record and stc_bn_bwd_apply_sync applies the sum of the ranks' records with the global count.
// All reductions are fixed-order => bitwise reproducible.
//
// Each piece is stated once and the kernels are thin users of it, but for the reduction layout, which
// chan_stats_kernel still repeats (see there):
//   ChunkReduce          the per-chunk reduction skeleton (chan_sum, bn_bwd_reduce)
//   WaveMerge/BlockMerge the two reduction policies of the chunk merges (bn_finalize, bn_bwd_finalize)
//   NoMask/PhiloxMask    the compile-time dropout policy (bn_bwd_reduce; the *_drop element-wise kernels)
//   bn_bwd_reduce_body   the backward's chunk reduction, with or without the dx store (bn_bwd_reduce, and
//                        bn_bwd_frozen_sums: running statistics, where that one pass is the whole backward)
//   bn_fwd_emit          the forward per element: n, the optional mask, one or two activations
//   bn_bwd_table/_dx     the backward per element: the k0/k1/k2 table (bn_bwd_coef: from loaded values) and dx from
//                        (v, g1, g2, mask); dn_term is one gradient's term of dn (dn_add: of a whole vector, as the
//                        reduce adds it)
//   bn_merge_stats / bn_bwd_merge  the two chunk merges as bodies, for the sync kernels (bn_finalize_kernel and
//                        bn_bwd_finalize_kernel keep their own, pinned, copies)
#include <type_traits>

#include "common.hpp"
#include "philox.hpp"
#include "vec16.hpp"

namespace stc {

constexpr int STAT_PIX = 64;  // pixels per statistics chunk (upper bound of chunk count below)

__host__ __device__ inline int stat_chunks(long long P) {
  long long c = (P + STAT_PIX - 1) / STAT_PIX;
  if (c > 1024) c = 1024;
  if (c < 1) c = 1;
  return (int)c;
}

// pixel index -> (b, y, x); exact float-reciprocal division below 2^24 pixels, integer division above
struct PixDiv {
  int HW, W;
  float inv_hw, inv_w;
  bool big;
};
static inline PixDiv mkpix(int B, int H, int W) {
  PixDiv d;
  d.HW = H * W; d.W = W;
  d.inv_hw = 1.f / (float)(H * W); d.inv_w = 1.f / (float)W;
  d.big = (long long)B * H * W >= (1ll << 24);
  return d;
}
__device__ __forceinline__ void pix_bxy(const PixDiv& d, long long pix, int& b, int& y, int& x) {
  int rem;
  if (d.big) {
    b = (int)(pix / d.HW);
    rem = (int)(pix - (long long)b * d.HW);
    y = rem / d.W;
  } else {
    const int pi = (int)pix;
    b = fast_div(pi, d.HW, d.inv_hw);
    rem = pi - b * d.HW;
    y = fast_div(rem, d.W, d.inv_w);
  }
  x = rem - y * d.W;
}

template <typename T>
__device__ __forceinline__ const T* vptr(const View& v, int b, int y, int x, int c) {
  return reinterpret_cast<const T*>(v.p) + vidx(v, b, y, x, c);
}

// (scale, shift) of the N channels from c; the identity without a table
template <int N>
__device__ __forceinline__ void ld_affine(const float* scale, const float* shift, int c, float* sc, float* sh) {
  if (scale) { ldc<N>(scale + c, sc); ldc<N>(shift + c, sh); }
  else {
#pragma unroll
    for (int e = 0; e < N; ++e) { sc[e] = 1.f; sh[e] = 0.f; }
  }
}

// ---- dropout policy of the kernels that exist with and without a mask (philox.hpp holds the mask function)
struct NoMask {
  static constexpr bool ON = false;
  struct Key {};
  __device__ __forceinline__ Key key() const { return Key{}; }
};
struct PhiloxMask {
  static constexpr bool ON = true;
  using Key = DropKey;
  DropDev d;
  __device__ __forceinline__ Key key() const { return drop_key(d); }
  // logical index of the vector's first element
  __device__ __forceinline__ unsigned long long index(int C, int b, int y, int x, int c) const {
    return drop_index(d, C, b, y, x, c);
  }
  template <int N>
  __device__ __forceinline__ void factor(const Key& k, unsigned long long li, float* m) const {
    drop_factor<N>(d, k, li, m);
  }
};

// Skeleton of the per-channel chunk reductions.  Thread = (channel group cg of N channels, pixel lane pl);
// block blockIdx.x owns the contiguous pixel range [p0, p1) and its RL lanes stride through it, each adding
// its pixels in order into its ROW accumulators; lane 0 of every channel group then adds the lanes' rows in
// lane order (fixed order).
template <int ROW>
struct ChunkReduce {
  int CG, RL, cg, pl;
  long long p0, p1;
  __device__ __forceinline__ ChunkReduce(long long P, int CG_, int nchunks)
      : CG(CG_), RL(256 / CG_), cg(threadIdx.x % CG_), pl(threadIdx.x / CG_) {
    const long long per = (P + nchunks - 1) / nchunks;
    p0 = blockIdx.x * per;
    p1 = min(P, p0 + per);
  }
  // init() once, then pixel(pix) for each of this lane's pixels; both add into the caller's acc[ROW].
  // Returns true on the pl == 0 threads, whose acc then holds the chunk's totals.
  template <class Init, class Pixel>
  __device__ __forceinline__ bool run(float* acc, Init&& init, Pixel&& pixel) {
    __shared__ float red[256][ROW];
    if (pl < RL) {
      init();
#pragma unroll 4
      for (long long pix = p0 + pl; pix < p1; pix += RL) pixel(pix);
    }
#pragma unroll
    for (int j = 0; j < ROW; ++j) red[threadIdx.x][j] = acc[j];
    __syncthreads();
    if (pl != 0) return false;
    float tot[ROW];  // (its own registers: summed into acc itself, the loop fills with register copies)
#pragma unroll
    for (int j = 0; j < ROW; ++j) tot[j] = 0.f;
    for (int k = 0; k < RL; ++k) {  // fixed order
      const int t = k * CG + cg;
#pragma unroll
      for (int j = 0; j < ROW; ++j) tot[j] += red[t][j];
    }
#pragma unroll
    for (int j = 0; j < ROW; ++j) acc[j] = tot[j];
    return true;
  }
};

// (chan_stats_kernel keeps its own copy of the ChunkReduce layout: through the skeleton its bf16 form took 25 % longer)
// part[chunk][c] = {n, S1, S2, shift}
template <typename T>
__global__ void __launch_bounds__(256) chan_stats_kernel(View x, PixDiv pd, long long P, int C, float* part, int nchunks) {
  constexpr int N = Vec16<T>::N;
  const int CG = C / N;
  const int RL = 256 / CG;
  const int cg = threadIdx.x % CG, pl = threadIdx.x / CG;
  const long long per = (P + nchunks - 1) / nchunks;
  const long long p0 = blockIdx.x * per, p1 = min(P, p0 + per);
  __shared__ float red[256][2 * N + 1];
  float s1[N], s2[N], sh[N], cnt = 0.f;
#pragma unroll
  for (int e = 0; e < N; ++e) { s1[e] = 0.f; s2[e] = 0.f; sh[e] = 0.f; }
  if (pl < RL && p0 < p1) {
    int b, yy, xx;
    pix_bxy(pd, p0, b, yy, xx);
    Vec16<T>::load(vptr<T>(x, b, yy, xx, N * cg), sh);
#pragma unroll 4
    for (long long pix = p0 + pl; pix < p1; pix += RL) {
      pix_bxy(pd, pix, b, yy, xx);
      float v[N];
      Vec16<T>::load(vptr<T>(x, b, yy, xx, N * cg), v);
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const float d = v[e] - sh[e];
        s1[e] += d;
        s2[e] += d * d;
      }
      cnt += 1.f;
    }
  }
#pragma unroll
  for (int e = 0; e < N; ++e) { red[threadIdx.x][e] = s1[e]; red[threadIdx.x][N + e] = s2[e]; }
  red[threadIdx.x][2 * N] = cnt;
  __syncthreads();
  if (pl == 0) {
    float a1[N], a2[N], n = 0.f;
#pragma unroll
    for (int e = 0; e < N; ++e) { a1[e] = 0.f; a2[e] = 0.f; }
    for (int k = 0; k < RL; ++k) {  // fixed order
      const int t = k * CG + cg;
#pragma unroll
      for (int e = 0; e < N; ++e) { a1[e] += red[t][e]; a2[e] += red[t][N + e]; }
      n += red[t][2 * N];
    }
#pragma unroll
    for (int e = 0; e < N; ++e)
      *reinterpret_cast<float4*>(part + ((long long)blockIdx.x * C + N * cg + e) * 4) = make_float4(n, a1[e], a2[e], sh[e]);
  }
}

// ---- reduction policies of the chunk merges: which lanes share a channel, and their fp64 total
// one wave per channel, 4 channels per block, no block barriers: a merge runs once per BatchNorm per pass, so
// its latency, not its bytes, is what it costs
struct WaveMerge {
  static constexpr int LANES = 64, CPB = 4;
  __device__ __forceinline__ static int lane() { return threadIdx.x & 63; }
  __device__ __forceinline__ static int channel() { return blockIdx.x * 4 + (threadIdx.x >> 6); }
  __device__ __forceinline__ static double sum(double v) { return wave_sum(v); }
};
// one block per channel (butterfly within each wave, then the 4 wave totals in a fixed order: deterministic, 2 barriers)
struct BlockMerge {
  static constexpr int LANES = 256, CPB = 1;
  __device__ __forceinline__ static int lane() { return threadIdx.x; }
  __device__ __forceinline__ static int channel() { return blockIdx.x; }
  __device__ __forceinline__ static double sum(double v) {
    __shared__ double sh[256];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return r;
  }
};
template <class R> static dim3 merge_grid(int C) { return dim3((C + R::CPB - 1) / R::CPB); }

// Merge of the per-chunk statistics {n, S1 = sum(x - shift), S2 = sum((x - shift)^2), shift}:
// chunk mean m_b = shift + S1/n, chunk M2_b = S2 - S1^2/n; then (exactly, in fp64)
//   mean = sum n_b m_b / N,   M2 = sum [M2_b + n_b (m_b - mean)^2]
// in two passes over the chunks (the policy's lanes per channel, fixed-order tree -> deterministic).
// The merge itself, for the kernels added after bn_finalize_kernel (which keeps its own copy below: through this body
// the compiler schedules it differently, and its code is pinned): pre_load(c), the caller's own loads for channel c,
// issued with the partials' loads; emit(c, N, mean, M2) on lane 0.
template <class R, class Pre, class Emit>
__device__ __forceinline__ void bn_merge_stats(const float* part, int nchunks, int C, Pre&& pre_load, Emit&& emit) {
  constexpr int L = R::LANES;
  const int lane = R::lane(), c = R::channel();
  if (R::CPB > 1 && c >= C) return;
  // chunk partials are read in groups of 4 per lane (the 4 loads in flight together: one
  // memory latency per group -- the first layers merge up to 4096 chunks per channel)
  auto load4 = [&](int k0, float4* pp) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * L;
      pp[u] = k < nchunks ? *reinterpret_cast<const float4*>(part + ((long long)k * C + c) * 4)
                          : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  pre_load(c);
  auto sum1 = [&](const float4* pp, double& n, double& sm) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (pp[u].x <= 0.f) continue;
      n += pp[u].x;
      sm += (double)pp[u].x * pp[u].w + (double)pp[u].y;  // n_b * m_b = n_b*shift + S1
    }
  };
  auto sum2 = [&](const float4* pp, double mu, double& m2) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (pp[u].x <= 0.f) continue;
      const double nb = pp[u].x, s1 = pp[u].y, r = s1 / nb;
      double q = (double)pp[u].z - s1 * r;
      if (q < 0) q = 0;
      const double d = (double)pp[u].w + r - mu;
      m2 += q + nb * d * d;
    }
  };
  // up to 16 L chunks: every lane loads its (up to) 4 groups of 4 partials at once and keeps them in registers
  // for both passes (one memory latency); the sums run in the loop's order below, so the results are the same
  auto in_regs = [&](auto Gc, double& n, double& sm, double& m2) {
    constexpr int G = decltype(Gc)::value;
    float4 pp[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g) load4(lane + 4 * L * g, pp[g]);
#pragma unroll
    for (int g = 0; g < G; ++g) sum1(pp[g], n, sm);
    n = R::sum(n);
    sm = R::sum(sm);
    const double mu = n > 0 ? sm / n : 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) sum2(pp[g], mu, m2);
    return mu;
  };
  double n = 0, sm = 0, m2 = 0, mu;
  if (nchunks <= 4 * L) {
    mu = in_regs(std::integral_constant<int, 1>{}, n, sm, m2);
  } else if (nchunks <= 8 * L) {
    mu = in_regs(std::integral_constant<int, 2>{}, n, sm, m2);
  } else if (nchunks <= 16 * L) {
    mu = in_regs(std::integral_constant<int, 4>{}, n, sm, m2);
  } else {
    for (int k0 = lane; k0 < nchunks; k0 += 4 * L) {
      float4 pp[4];
      load4(k0, pp);
      sum1(pp, n, sm);
    }
    n = R::sum(n);
    sm = R::sum(sm);
    mu = n > 0 ? sm / n : 0.0;
    for (int k0 = lane; k0 < nchunks; k0 += 4 * L) {
      float4 pp[4];
      load4(k0, pp);
      sum2(pp, mu, m2);
    }
  }
  const double M2 = R::sum(m2);
  if (lane == 0) emit(c, n, mu, M2);
}

template <class R>
__global__ void __launch_bounds__(256) bn_finalize_kernel(const float* part, int nchunks, int C,
                                                          const float* gamma, const float* beta,
                                                          float* rmean, float* rvar, long long* nbt,
                                                          float momentum, float eps,
                                                          float* mean_o, float* rstd_o, float* scale, float* shift) {
  constexpr int L = R::LANES;
  const int lane = R::lane(), c = R::channel();
  if (R::CPB > 1 && c >= C) return;
  // chunk partials are read in groups of 4 per lane (the 4 loads in flight together: one
  // memory latency per group -- the first layers merge up to 4096 chunks per channel)
  auto load4 = [&](int k0, float4* pp) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * L;
      pp[u] = k < nchunks ? *reinterpret_cast<const float4*>(part + ((long long)k * C + c) * 4)
                          : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  const BnPre pre = bn_pre(c, gamma, beta, rmean, rvar);  // (issued with the partials' loads)
  auto sum1 = [&](const float4* pp, double& n, double& sm) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (pp[u].x <= 0.f) continue;
      n += pp[u].x;
      sm += (double)pp[u].x * pp[u].w + (double)pp[u].y;  // n_b * m_b = n_b*shift + S1
    }
  };
  auto sum2 = [&](const float4* pp, double mu, double& m2) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (pp[u].x <= 0.f) continue;
      const double nb = pp[u].x, s1 = pp[u].y, r = s1 / nb;
      double q = (double)pp[u].z - s1 * r;
      if (q < 0) q = 0;
      const double d = (double)pp[u].w + r - mu;
      m2 += q + nb * d * d;
    }
  };
  // up to 16 L chunks: every lane loads its (up to) 4 groups of 4 partials at once and keeps them in registers
  // for both passes (one memory latency); the sums run in the loop's order below, so the results are the same
  auto in_regs = [&](auto Gc, double& n, double& sm, double& m2) {
    constexpr int G = decltype(Gc)::value;
    float4 pp[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g) load4(lane + 4 * L * g, pp[g]);
#pragma unroll
    for (int g = 0; g < G; ++g) sum1(pp[g], n, sm);
    n = R::sum(n);
    sm = R::sum(sm);
    const double mu = n > 0 ? sm / n : 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) sum2(pp[g], mu, m2);
    return mu;
  };
  double n = 0, sm = 0, m2 = 0, mu;
  if (nchunks <= 4 * L) {
    mu = in_regs(std::integral_constant<int, 1>{}, n, sm, m2);
  } else if (nchunks <= 8 * L) {
    mu = in_regs(std::integral_constant<int, 2>{}, n, sm, m2);
  } else if (nchunks <= 16 * L) {
    mu = in_regs(std::integral_constant<int, 4>{}, n, sm, m2);
  } else {
    for (int k0 = lane; k0 < nchunks; k0 += 4 * L) {
      float4 pp[4];
      load4(k0, pp);
      sum1(pp, n, sm);
    }
    n = R::sum(n);
    sm = R::sum(sm);
    mu = n > 0 ? sm / n : 0.0;
    for (int k0 = lane; k0 < nchunks; k0 += 4 * L) {
      float4 pp[4];
      load4(k0, pp);
      sum2(pp, mu, m2);
    }
  }
  const double M2 = R::sum(m2);
  if (lane == 0) bn_finalize_store(c, n, mu, M2, pre, rmean, rvar, nbt, momentum, eps, mean_o, rstd_o, scale, shift);
}

// Sync statistics: one rank's chunk partials merged into ONE record per channel, in the partials' own format, so that
// stc_bn_finalize over the ranks' records (nchunks = world) gives the statistics of the global batch.  From the merged
// (N, mean, M2), all fp64: shift = fl32(mean), d = mean - shift (|d| <= ulp(mean)/2),
//   rec = {N, S1 = N d, S2 = M2 + N d^2, shift}
// which the merge reads back as mean_b = shift + S1/N = mean and M2_b = S2 - S1^2/N = M2: exactly, but for the fp32
// rounding of S1 (a relative 2^-24 of at most half an ulp of the mean) and of S2 (a relative 2^-24 of M2).  N is
// exact below 2^24 pixels per rank.
template <class R>
__global__ void __launch_bounds__(256) bn_stats_pack_kernel(const float* part, int nchunks, int C, float* rec) {
  bn_merge_stats<R>(part, nchunks, C, [](int) {}, [&](int c, double n, double mu, double M2) {
    const float sh = (float)mu;
    const double d = mu - (double)sh;
    *reinterpret_cast<float4*>(rec + (long long)c * 4) = make_float4((float)n, (float)(n * d), (float)(M2 + n * d * d), sh);
  });
}

// eval-mode table from running statistics
__global__ void bn_eval_table_kernel(int C, const float* gamma, const float* beta, const float* rmean,
                                     const float* rvar, float eps, float* scale, float* shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float rs = 1.f / sqrtf(rvar[c] + eps);
  const float sc = gamma[c] * rs;
  scale[c] = sc;
  shift[c] = beta[c] - rmean[c] * sc;
}

struct GradIn {
  View g1, g2;
  float s1, s2;
  int has1, has2;
};

// One gradient's term of dn = g1*act1'(n) + g2*act2'(n); MASKED: g reaches n through the dropout, g * keep/(1-p)
template <bool MASKED>
__device__ __forceinline__ float dn_term(float g, float m, float n, float slope) {
  if constexpr (MASKED) return (g * m) * dact(n, slope);
  else return g * dact(n, slope);
}
// ... of a whole vector (the reduce adds a gradient's term right after that gradient's load)
template <int N, bool MASKED>
__device__ __forceinline__ void dn_add(const float* g, const float* m, const float* n, float slope, float* dn) {
#pragma unroll
  for (int e = 0; e < N; ++e) dn[e] += dn_term<MASKED>(g[e], MASKED ? m[e] : 1.f, n[e], slope);
}

// The backward per element, for the N channels from c:
// n = v*sc + sh;  dx = k1*dn - k0 - k2*v   with k1 = gamma*rstd, k2 = k1*rstd*dgamma/P,
// k0 = k1*(dbeta/P - mean*rstd*dgamma/P); without mean (activation only) dx = dn.
// MASKED: g1 is required and carries the dropout factor m.
// CHECKED = false: the entry point has required every table (the _drop calls), so the tests for an absent scale or
// mean are compiled out -- behind them the compiler contracts k0's products differently and dx's last bit moves.
template <int N>
__device__ __forceinline__ void bn_bwd_coef(const float* mu, const float* rs, const float* gm, const float* dg,
                                            const float* db, float invP, float* k0, float* k1, float* k2) {
#pragma unroll
  for (int e = 0; e < N; ++e) {
    k1[e] = gm[e] * rs[e];
    k2[e] = k1[e] * rs[e] * dg[e] * invP;
    k0[e] = k1[e] * (db[e] * invP - mu[e] * rs[e] * dg[e] * invP);
  }
}
template <int N, bool CHECKED = true>
__device__ __forceinline__ void bn_bwd_table(int c, const float* scale, const float* shift, const float* mean,
                                             const float* rstd, const float* gamma, const float* dgamma,
                                             const float* dbeta, float invP, float* sc, float* sh, float* k0,
                                             float* k1, float* k2) {
  if (CHECKED) ld_affine<N>(scale, shift, c, sc, sh);
  else { ldc<N>(scale + c, sc); ldc<N>(shift + c, sh); }
  if (!CHECKED || mean) {
    float mu[N], rs[N], gm[N], dg[N], db[N];
    ldc<N>(mean + c, mu); ldc<N>(rstd + c, rs); ldc<N>(gamma + c, gm); ldc<N>(dgamma + c, dg); ldc<N>(dbeta + c, db);
    bn_bwd_coef<N>(mu, rs, gm, dg, db, invP, k0, k1, k2);
  } else {
#pragma unroll
    for (int e = 0; e < N; ++e) { k1[e] = 1.f; k2[e] = 0.f; k0[e] = 0.f; }
  }
}
template <int N, bool MASKED>
__device__ __forceinline__ void bn_bwd_dx(const GradIn& gi, const float* sc, const float* sh, const float* k0,
                                          const float* k1, const float* k2, const float* v, const float* g1,
                                          const float* g2, const float* m, float* d) {
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const float n = fmaf(v[e], sc[e], sh[e]);
    float dn = 0.f;
    if constexpr (MASKED) dn += dn_term<true>(g1[e], m[e], n, gi.s1);
    else if (gi.has1) dn += dn_term<false>(g1[e], 1.f, n, gi.s1);
    if (gi.has2) dn += dn_term<false>(g2[e], 1.f, n, gi.s2);
    d[e] = fmaf(k1[e], dn, -fmaf(k2[e], v[e], k0[e]));
  }
}

// part2[chunk][c] = {sum dn, sum dn*xhat}.  With PhiloxMask g1 is required and no mask is stored: it is
// recomputed from the call's counter.  DX (frozen statistics, bn_bwd_frozen_sums_kernel): the pass also stores
// dx = scale * dn, which with fixed mean / rstd is the whole input gradient.
template <typename T, class M, bool DX>
__device__ __forceinline__ void bn_bwd_reduce_body(const View& x, const PixDiv& pd, long long P, int C,
                                                   const float* scale, const float* shift, const float* mean,
                                                   const float* rstd, const GradIn& gi, float* part, int nchunks,
                                                   const M& mask, const View& dx) {
  constexpr int N = Vec16<T>::N;
  ChunkReduce<2 * N> r(P, C / N, nchunks);
  const int c = N * r.cg;
  float acc[2 * N], sc[N], shf[N], mu[N], rs[N];  // acc = {sum dn [N], sum dn*xhat [N]}
  typename M::Key key;
#pragma unroll
  for (int j = 0; j < 2 * N; ++j) acc[j] = 0.f;
  const bool lead = r.run(
      acc,
      [&] {
        key = mask.key();
        ldc<N>(scale + c, sc); ldc<N>(shift + c, shf); ldc<N>(mean + c, mu); ldc<N>(rstd + c, rs);
      },
      // (4 pixels' loads and Philox rounds in flight together; the sums stay in pixel order)
      [&](long long pix) {
        int b, yy, xx;
        pix_bxy(pd, pix, b, yy, xx);
        float v[N], n[N], d[N];
        Vec16<T>::load(vptr<T>(x, b, yy, xx, c), v);
#pragma unroll
        for (int e = 0; e < N; ++e) { n[e] = fmaf(v[e], sc[e], shf[e]); d[e] = 0.f; }
        if (M::ON || gi.has1) {
          float g[N], m[N];
          Vec16<T>::load(vptr<T>(gi.g1, b, yy, xx, c), g);
          if constexpr (M::ON) mask.template factor<N>(key, mask.index(C, b, yy, xx, c), m);
          dn_add<N, M::ON>(g, m, n, gi.s1, d);
        }
        if (gi.has2) {
          float g[N];
          Vec16<T>::load(vptr<T>(gi.g2, b, yy, xx, c), g);
          dn_add<N, false>(g, nullptr, n, gi.s2, d);
        }
        if constexpr (DX) {
          float o[N];
#pragma unroll
          for (int e = 0; e < N; ++e) o[e] = sc[e] * d[e];
          Vec16<T>::store(reinterpret_cast<T*>(dx.p) + vidx(dx, b, yy, xx, c), o);
        }
#pragma unroll
        for (int e = 0; e < N; ++e) {
          acc[e] += d[e];
          acc[N + e] += d[e] * (v[e] - mu[e]) * rs[e];
        }
      });
  if (lead) {
#pragma unroll
    for (int e = 0; e < N; ++e)
      *reinterpret_cast<float2*>(part + ((long long)blockIdx.x * C + c + e) * 2) = make_float2(acc[e], acc[N + e]);
  }
}

template <typename T, class M>
__global__ void __launch_bounds__(256) bn_bwd_reduce_kernel(View x, PixDiv pd, long long P, int C, const float* scale,
                                                            const float* shift, const float* mean, const float* rstd,
                                                            GradIn gi, float* part, int nchunks, M mask) {
  bn_bwd_reduce_body<T, M, false>(x, pd, P, C, scale, shift, mean, rstd, gi, part, nchunks, mask, x);
}

// Frozen statistics (the layer normalised with its running statistics; scale / shift = the eval table, mean / rstd =
// running_mean / rstd_run): the reduce above that also writes dx -- one pass where the train-mode backward takes a
// reduce, a merge and an apply.  bn_bwd_finalize_kernel merges the partials as there.
template <typename T, class M>
__global__ void __launch_bounds__(256) bn_bwd_frozen_sums_kernel(View x, PixDiv pd, long long P, int C,
                                                                 const float* scale, const float* shift,
                                                                 const float* mean, const float* rstd, GradIn gi,
                                                                 float* part, int nchunks, View dx, M mask) {
  bn_bwd_reduce_body<T, M, true>(x, pd, P, C, scale, shift, mean, rstd, gi, part, nchunks, mask, dx);
}

// dbeta[c] = sum dn, dgamma[c] = sum dn*xhat  (fixed order over chunks, the policy's lanes per channel)
// (the merge of bn_bwd_finalize_kernel, which keeps its own copy for the same reason as bn_finalize_kernel:)
// emit(c, sum dn, sum dn*xhat) on lane 0
template <class R, class Emit>
__device__ __forceinline__ void bn_bwd_merge(const float* part, int nchunks, int C, Emit&& emit) {
  constexpr int L = R::LANES;
  const int lane = R::lane(), c = R::channel();
  if (R::CPB > 1 && c >= C) return;
  double a = 0, b = 0;
  for (int k0 = lane; k0 < nchunks; k0 += 4 * L) {  // groups of 4 loads in flight
    float2 pp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * L;
      pp[u] = k < nchunks ? *reinterpret_cast<const float2*>(part + ((long long)k * C + c) * 2) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a += pp[u].x;
      b += pp[u].y;
    }
  }
  a = R::sum(a);
  b = R::sum(b);
  if (lane == 0) emit(c, a, b);
}

template <class R>
__global__ void __launch_bounds__(256) bn_bwd_finalize_kernel(const float* part, int nchunks, int C, float* dgamma,
                                                              float* dbeta) {
  constexpr int L = R::LANES;
  const int lane = R::lane(), c = R::channel();
  if (R::CPB > 1 && c >= C) return;
  double a = 0, b = 0;
  for (int k0 = lane; k0 < nchunks; k0 += 4 * L) {  // groups of 4 loads in flight
    float2 pp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * L;
      pp[u] = k < nchunks ? *reinterpret_cast<const float2*>(part + ((long long)k * C + c) * 2) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a += pp[u].x;
      b += pp[u].y;
    }
  }
  a = R::sum(a);
  b = R::sum(b);
  if (lane == 0) {
    dbeta[c] = (float)a;
    dgamma[c] = (float)b;
  }
}

// Sync statistics: the same merge; this rank's dbeta / dgamma (absent: no parameter gradient wanted) and the record
// rec[c] = {sum dn, sum dn*xhat}, the same fp32 values, for the exchange
template <class R>
__global__ void __launch_bounds__(256) bn_bwd_sums_kernel(const float* part, int nchunks, int C, float* dgamma,
                                                          float* dbeta, float* rec) {
  bn_bwd_merge<R>(part, nchunks, C, [&](int c, double a, double b) {
    if (dgamma) {
      dbeta[c] = (float)a;
      dgamma[c] = (float)b;
    }
    *reinterpret_cast<float2*>(rec + (long long)c * 2) = make_float2((float)a, (float)b);
  });
}

template <typename T, bool DENSE>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(View x, PixDiv pd, long long P, int C, const float* scale,
                                                           const float* shift, const float* mean, const float* rstd,
                                                           const float* gamma, GradIn gi, const float* dgamma,
                                                           const float* dbeta, View dx) {
  constexpr int N = Vec16<T>::N;
  const int CG = C / N;
  const long long total = P * CG;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const float invP = 1.f / (float)P;
  // per-channel coefficients of this thread's channel group, reloaded only when the group changes
  // (never, when the grid stride is a multiple of CG -- the usual power-of-two channel counts):
  // n = v*sc + sh;  dx = k1*dn - k0 - k2*v   with k1 = gamma*rstd, k2 = k1*rstd*dgamma/P,
  // k0 = k1*(dbeta/P - mean*rstd*dgamma/P)
  int cg_have = -1;
  float sc[N], sh[N], k0[N], k1[N], k2[N];
  auto table = [&](int cg) {
    if (cg == cg_have) return;
    cg_have = cg;
    bn_bwd_table<N>(N * cg, scale, shift, mean, rstd, gamma, dgamma, dbeta, invP, sc, sh, k0, k1, k2);
  };
  struct Off {
    long long x, g1, g2, dx;
    int c;
  };
  auto offs = [&](long long idx) {
    Off o;
    const int cg = (int)(idx % CG);
    const long long pix = idx / CG;
    o.c = N * cg;
    if constexpr (DENSE) {
      o.x = pix * x.ps + x.co + o.c;
      o.g1 = pix * gi.g1.ps + gi.g1.co + o.c;
      o.g2 = pix * gi.g2.ps + gi.g2.co + o.c;
      o.dx = pix * dx.ps + dx.co + o.c;
    } else {
      int b, yy, xx;
      pix_bxy(pd, pix, b, yy, xx);
      o.x = vidx(x, b, yy, xx, o.c);
      o.g1 = vidx(gi.g1, b, yy, xx, o.c);
      o.g2 = vidx(gi.g2, b, yy, xx, o.c);
      o.dx = vidx(dx, b, yy, xx, o.c);
    }
    return o;
  };
  struct In {
    float v[N], g1[N], g2[N];
  };
  auto load = [&](const Off& o, In& in) {
    Vec16<T>::load(reinterpret_cast<const T*>(x.p) + o.x, in.v);
    if (gi.has1) Vec16<T>::load(reinterpret_cast<const T*>(gi.g1.p) + o.g1, in.g1);
    if (gi.has2) Vec16<T>::load(reinterpret_cast<const T*>(gi.g2.p) + o.g2, in.g2);
  };
  auto emit = [&](const Off& o, const In& in) {
    table(o.c / N);
    float d[N];
    bn_bwd_dx<N, false>(gi, sc, sh, k0, k1, k2, in.v, in.g1, in.g2, nullptr, d);
    Vec16<T>::store(reinterpret_cast<T*>(dx.p) + o.dx, d);
  };
  if constexpr (DENSE) {
    // Streaming form (host: every view pixel-dense with 32-bit element offsets, 256 % CG == 0, so
    // the grid stride is a whole number of pixels): this thread's channel group and its table are
    // fixed, the pixel advances by a constant -- no per-element index division.
    const unsigned nthr = gridDim.x * blockDim.x, t0 = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned pstep = nthr / (unsigned)CG, Pu = (unsigned)P;
    unsigned pix = t0 / (unsigned)CG;
    if (pix >= Pu) return;
    const int c = N * (int)(t0 % (unsigned)CG);
    table(c / N);
    const T* xp = reinterpret_cast<const T*>(x.p) + x.co + c;
    const T* g1p = reinterpret_cast<const T*>(gi.g1.p) + gi.g1.co + c;
    const T* g2p = reinterpret_cast<const T*>(gi.g2.p) + gi.g2.co + c;
    T* dp = reinterpret_cast<T*>(dx.p) + dx.co + c;
    const unsigned xs = x.ps, g1s = gi.g1.ps, g2s = gi.g2.ps, ds = dx.ps;
    auto ld = [&](unsigned q, In& in) {
      Vec16<T>::load(xp + q * xs, in.v);
      if (gi.has1) Vec16<T>::load(g1p + q * g1s, in.g1);
      if (gi.has2) Vec16<T>::load(g2p + q * g2s, in.g2);
    };
    auto put = [&](unsigned q, const In& in) {
      float d[N];
      bn_bwd_dx<N, false>(gi, sc, sh, k0, k1, k2, in.v, in.g1, in.g2, nullptr, d);
      Vec16<T>::store(dp + q * ds, d);
    };
    for (; pix + pstep < Pu; pix += 2 * pstep) {  // both pixels' loads in flight before either is used
      In a, b;
      ld(pix, a);
      ld(pix + pstep, b);
      put(pix, a);
      put(pix + pstep, b);
    }
    if (pix < Pu) {
      In a;
      ld(pix, a);
      put(pix, a);
    }
    return;
  }
  long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; idx + stride < total; idx += 2 * stride) {  // both elements' loads in flight before either is used
    const Off oa = offs(idx), ob = offs(idx + stride);
    In a, b;
    load(oa, a);
    load(ob, b);
    emit(oa, a);
    emit(ob, b);
  }
  if (idx < total) {
    const Off oa = offs(idx);
    In a;
    load(oa, a);
    emit(oa, a);
  }
}

// The forward per element: n = v0*sc + sh, the dropout factor when MASKED (kept: n * keep/(1-p), dropped: 0; it
// sits between the affine and the activations, in fp32), then y1 = act(n, s1) and optionally y2 = act(n, s2)
template <typename T, bool MASKED>
__device__ __forceinline__ void bn_fwd_emit(const float* v0, const float* sc, const float* sh, const float* m,
                                            const View& y1, long long o1, float s1, const View& y2, long long o2,
                                            float s2, int has2) {
  constexpr int N = Vec16<T>::N;
  float v[N], o[N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const float n = fmaf(v0[e], sc[e], sh[e]);
    if constexpr (MASKED) v[e] = m[e] != 0.f ? n * m[e] : 0.f;
    else v[e] = n;
  }
#pragma unroll
  for (int e = 0; e < N; ++e) o[e] = act(v[e], s1);
  Vec16<T>::store(reinterpret_cast<T*>(y1.p) + o1, o);
  if (has2) {
#pragma unroll
    for (int e = 0; e < N; ++e) o[e] = act(v[e], s2);
    Vec16<T>::store(reinterpret_cast<T*>(y2.p) + o2, o);
  }
}

// Activation materialisation: n = x*scale + shift (identity without a table), then
// y1 = act(n, slope1) and optionally y2 = act(n, slope2) (slope 0 = ReLU, 0.2 = the
// LeakyReLU of the reference, 1 = identity).  Applied once per element, so the GEMMs
// that consume y1/y2 (each input element is re-read 4-16x by the im2col) stage plain
// operands with no per-load transform.
template <typename T, bool DENSE>
__global__ void __launch_bounds__(256) bn_apply_kernel(View x, PixDiv pd, long long P, int C, const float* scale,
                                                       const float* shift, View y1, float s1, View y2, float s2,
                                                       int has2) {
  constexpr int N = Vec16<T>::N;
  const int CG = C / N;
  const long long total = P * CG;
  const long long stride = (long long)gridDim.x * blockDim.x;
  int cg_have = -1;
  float sc[N], sh[N];
  auto table = [&](int cg) {  // this thread's channel group's table, reloaded only when it changes
    if (cg == cg_have) return;
    cg_have = cg;
    ld_affine<N>(scale, shift, N * cg, sc, sh);
  };
  auto offs = [&](long long idx, long long& ox, long long& o1, long long& o2, int& c) {
    const int cg = (int)(idx % CG);
    const long long pix = idx / CG;
    c = N * cg;
    if constexpr (DENSE) {  // every view dense in pixels: element (pix, c) at pix*ps + co + c
      ox = pix * x.ps + x.co + c;
      o1 = pix * y1.ps + y1.co + c;
      o2 = pix * y2.ps + y2.co + c;
    } else {
      int b, yy, xx;
      pix_bxy(pd, pix, b, yy, xx);
      ox = vidx(x, b, yy, xx, c);
      o1 = vidx(y1, b, yy, xx, c);
      o2 = vidx(y2, b, yy, xx, c);
    }
  };
  auto emit = [&](const float* v0, long long o1, long long o2) {
    bn_fwd_emit<T, false>(v0, sc, sh, nullptr, y1, o1, s1, y2, o2, s2, has2);
  };
  if constexpr (DENSE) {  // streaming form: as bn_bwd_apply_kernel's
    const unsigned nthr = gridDim.x * blockDim.x, t0 = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned pstep = nthr / (unsigned)CG, Pu = (unsigned)P;
    unsigned pix = t0 / (unsigned)CG;
    if (pix >= Pu) return;
    const int c = N * (int)(t0 % (unsigned)CG);
    table(c / N);
    const T* xp = reinterpret_cast<const T*>(x.p) + x.co + c;
    const unsigned xs = x.ps, s1s = y1.ps, s2s = y2.ps;
    const long long b1 = y1.co + c, b2 = y2.co + c;
    for (; pix + pstep < Pu; pix += 2 * pstep) {
      float va[N], vb[N];
      Vec16<T>::load(xp + pix * xs, va);
      Vec16<T>::load(xp + (pix + pstep) * xs, vb);
      emit(va, b1 + pix * s1s, b2 + pix * s2s);
      emit(vb, b1 + (pix + pstep) * s1s, b2 + (pix + pstep) * s2s);
    }
    if (pix < Pu) {
      float va[N];
      Vec16<T>::load(xp + pix * xs, va);
      emit(va, b1 + pix * s1s, b2 + pix * s2s);
    }
    return;
  }
  long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; idx + stride < total; idx += 2 * stride) {  // two 16-byte loads in flight per thread
    long long ax, a1, a2, bx, b1, b2;
    int ca, cb;
    offs(idx, ax, a1, a2, ca);
    offs(idx + stride, bx, b1, b2, cb);
    float va[N], vb[N];
    Vec16<T>::load(reinterpret_cast<const T*>(x.p) + ax, va);
    Vec16<T>::load(reinterpret_cast<const T*>(x.p) + bx, vb);
    table(ca / N);
    emit(va, a1, a2);
    table(cb / N);
    emit(vb, b1, b2);
  }
  if (idx < total) {
    long long ax, a1, a2;
    int ca;
    offs(idx, ax, a1, a2, ca);
    float va[N];
    Vec16<T>::load(reinterpret_cast<const T*>(x.p) + ax, va);
    table(ca / N);
    emit(va, a1, a2);
  }
}

// part[chunk][c] = sum over the chunk's pixels of x (conv bias gradients)
template <typename T>
__global__ void __launch_bounds__(256) chan_sum_kernel(View x, PixDiv pd, long long P, int C, float* part, int nchunks) {
  constexpr int N = Vec16<T>::N;
  ChunkReduce<N> r(P, C / N, nchunks);
  const int c = N * r.cg;
  float acc[N];
#pragma unroll
  for (int e = 0; e < N; ++e) acc[e] = 0.f;
  const bool lead = r.run(acc, [] {}, [&](long long pix) {
    int b, yy, xx;
    pix_bxy(pd, pix, b, yy, xx);
    float v[N];
    Vec16<T>::load(vptr<T>(x, b, yy, xx, c), v);
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] += v[e];
  });
  if (lead) {
#pragma unroll
    for (int e = 0; e < N; ++e) part[(long long)blockIdx.x * C + c + e] = acc[e];
  }
}

__global__ void chan_sum_final_kernel(const float* part, int nchunks, int C, int Cout, float* out) {
  const int c = blockIdx.x;
  __shared__ double s[256];
  double a = 0;
  for (int k = threadIdx.x; k < nchunks; k += 256) a += part[(long long)k * C + c];
  s[threadIdx.x] = a;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0 && c < Cout) out[c] = (float)s[0];
}

static GradIn mkgrad(stc_view g1, float s1, stc_view g2, float s2) {
  GradIn gi{};
  gi.has1 = g1.p != nullptr; gi.has2 = g2.p != nullptr;
  if (gi.has1) gi.g1 = mkview(g1);
  if (gi.has2) gi.g2 = mkview(g2);
  gi.s1 = s1; gi.s2 = s2;
  return gi;
}

// ---------------------------------------------------------------- dropout (use_dropout=True generators)
// The two element-wise kernels below are the general-addressing forms of bn_apply_kernel and bn_bwd_apply_kernel
// with the mask applied: the same per-element definitions, so that with every element kept at scale 1 they write
// what those kernels write.  The mask needs (b, y, x) of every vector, and the tensors it touches are small
// (<= 8 MB at bs 32): no streaming form.

// y = act(n * keep/(1-p), slope)
template <typename T>
__global__ void __launch_bounds__(256) bn_apply_drop_kernel(View x, PixDiv pd, long long P, int C, const float* scale,
                                                            const float* shift, View y1, float s1, View y2, float s2,
                                                            int has2, PhiloxMask mask) {
  constexpr int N = Vec16<T>::N;
  const int CG = C / N;
  const long long total = P * CG;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const DropKey key = mask.key();
  struct Off {
    long long x, y1, y2;
    unsigned long long li;  // logical index of the vector's first element
    int c;
  };
  auto offs = [&](long long idx) {
    Off o;
    const int cg = (int)(idx % CG);
    const long long pix = idx / CG;
    o.c = N * cg;
    int b, yy, xx;
    pix_bxy(pd, pix, b, yy, xx);
    o.x = vidx(x, b, yy, xx, o.c);
    o.y1 = vidx(y1, b, yy, xx, o.c);
    o.y2 = vidx(y2, b, yy, xx, o.c);
    o.li = mask.index(C, b, yy, xx, o.c);
    return o;
  };
  auto emit = [&](const Off& o, const float* v0) {
    float sc[N], sh[N], m[N];
    ld_affine<N>(scale, shift, o.c, sc, sh);
    mask.template factor<N>(key, o.li, m);
    bn_fwd_emit<T, true>(v0, sc, sh, m, y1, o.y1, s1, y2, o.y2, s2, has2);
  };
  long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; idx + stride < total; idx += 2 * stride) {  // two 16-byte loads in flight per thread
    const Off oa = offs(idx), ob = offs(idx + stride);
    float va[N], vb[N];
    Vec16<T>::load(reinterpret_cast<const T*>(x.p) + oa.x, va);
    Vec16<T>::load(reinterpret_cast<const T*>(x.p) + ob.x, vb);
    emit(oa, va);
    emit(ob, vb);
  }
  if (idx < total) {
    const Off oa = offs(idx);
    float va[N];
    Vec16<T>::load(reinterpret_cast<const T*>(x.p) + oa.x, va);
    emit(oa, va);
  }
}

// bn_bwd_apply_kernel (with the BN tables) and the masked g1
template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_apply_drop_kernel(View x, PixDiv pd, long long P, int C,
                                                                const float* scale, const float* shift,
                                                                const float* mean, const float* rstd,
                                                                const float* gamma, GradIn gi, const float* dgamma,
                                                                const float* dbeta, View dx, PhiloxMask mask) {
  constexpr int N = Vec16<T>::N;
  const int CG = C / N;
  const long long total = P * CG;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const float invP = 1.f / (float)P;
  const DropKey key = mask.key();
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int c = N * (int)(idx % CG);
    int b, yy, xx;
    pix_bxy(pd, idx / CG, b, yy, xx);
    float v[N], g1[N], g2[N], m[N], d[N];
    Vec16<T>::load(vptr<T>(x, b, yy, xx, c), v);
    Vec16<T>::load(vptr<T>(gi.g1, b, yy, xx, c), g1);
    if (gi.has2) Vec16<T>::load(vptr<T>(gi.g2, b, yy, xx, c), g2);
    float sc[N], sh[N], k0[N], k1[N], k2[N];
    bn_bwd_table<N, false>(c, scale, shift, mean, rstd, gamma, dgamma, dbeta, invP, sc, sh, k0, k1, k2);
    mask.template factor<N>(key, mask.index(C, b, yy, xx, c), m);
    bn_bwd_dx<N, true>(gi, sc, sh, k0, k1, k2, v, g1, g2, m, d);
    Vec16<T>::store(reinterpret_cast<T*>(dx.p) + vidx(dx, b, yy, xx, c), d);
  }
}

// Sync statistics (the batch spread over `world` data-parallel ranks): bn_bwd_apply_kernel / bn_bwd_apply_drop_kernel
// with the sums of the GLOBAL batch -- each thread adds the ranks' records {sum dn, sum dn*xhat} of its channels in
// rank order (fp64, then fp32: with one record, that record) -- and 1 / count, the global pixel count, for 1 / P.
// General addressing, as the _drop kernel: the layers that run it carry one small collective each anyway.
template <typename T, class M>
__global__ void __launch_bounds__(256) bn_bwd_apply_sync_kernel(View x, PixDiv pd, long long P, int C,
                                                                const float* scale, const float* shift,
                                                                const float* mean, const float* rstd,
                                                                const float* gamma, GradIn gi, const float* recs,
                                                                int world, long long count, View dx, M mask) {
  constexpr int N = Vec16<T>::N;
  const int CG = C / N;
  const long long total = P * CG;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const float invP = 1.f / (float)count;
  const typename M::Key key = mask.key();
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int c = N * (int)(idx % CG);
    int b, yy, xx;
    pix_bxy(pd, idx / CG, b, yy, xx);
    float v[N], g1[N], g2[N], m[N], d[N];
    Vec16<T>::load(vptr<T>(x, b, yy, xx, c), v);
    if (M::ON || gi.has1) Vec16<T>::load(vptr<T>(gi.g1, b, yy, xx, c), g1);
    if (gi.has2) Vec16<T>::load(vptr<T>(gi.g2, b, yy, xx, c), g2);
    float sc[N], sh[N], mu[N], rs[N], gm[N], dg[N], db[N], k0[N], k1[N], k2[N];
    ldc<N>(scale + c, sc); ldc<N>(shift + c, sh);
    ldc<N>(mean + c, mu); ldc<N>(rstd + c, rs); ldc<N>(gamma + c, gm);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      double a = 0, q = 0;
      for (int r = 0; r < world; ++r) {  // rank order: every rank forms the same sums
        const float2 s = *reinterpret_cast<const float2*>(recs + ((long long)r * C + c + e) * 2);
        a += s.x;
        q += s.y;
      }
      db[e] = (float)a;
      dg[e] = (float)q;
    }
    bn_bwd_coef<N>(mu, rs, gm, dg, db, invP, k0, k1, k2);
    if constexpr (M::ON) mask.template factor<N>(key, mask.index(C, b, yy, xx, c), m);
    bn_bwd_dx<N, M::ON>(gi, sc, sh, k0, k1, k2, v, g1, g2, m, d);
    Vec16<T>::store(reinterpret_cast<T*>(dx.p) + vidx(dx, b, yy, xx, c), d);
  }
}

// Frozen statistics, no parameter gradient wanted: dx = scale * dn alone, a plain streaming pass (no sums, no
// partials).  DENSE: the streaming form of bn_bwd_apply_kernel (no mask: it needs (b, y, x) of every vector);
// otherwise general addressing, with the dropout factor on g1 under PhiloxMask.
template <typename T, bool DENSE, class M>
__global__ void __launch_bounds__(256) bn_bwd_frozen_kernel(View x, PixDiv pd, long long P, int C, const float* scale,
                                                            const float* shift, GradIn gi, View dx, M mask) {
  static_assert(!(DENSE && M::ON), "the streaming form has no pixel coordinates for the mask");
  constexpr int N = Vec16<T>::N;
  const int CG = C / N;
  struct In {
    float v[N], g1[N], g2[N];
  };
  // dn as the reduce forms it (the same terms in the same order), then dx
  auto dx_of = [&](const In& in, const float* sc, const float* sh, const float* m, float* d) {
    float n[N], dn[N];
#pragma unroll
    for (int e = 0; e < N; ++e) { n[e] = fmaf(in.v[e], sc[e], sh[e]); dn[e] = 0.f; }
    if (M::ON || gi.has1) dn_add<N, M::ON>(in.g1, m, n, gi.s1, dn);
    if (gi.has2) dn_add<N, false>(in.g2, nullptr, n, gi.s2, dn);
#pragma unroll
    for (int e = 0; e < N; ++e) d[e] = sc[e] * dn[e];
  };
  if constexpr (DENSE) {  // (host: stream_ok for every view)
    const unsigned nthr = gridDim.x * blockDim.x, t0 = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned pstep = nthr / (unsigned)CG, Pu = (unsigned)P;
    unsigned pix = t0 / (unsigned)CG;
    if (pix >= Pu) return;
    const int c = N * (int)(t0 % (unsigned)CG);
    float sc[N], sh[N];
    ldc<N>(scale + c, sc); ldc<N>(shift + c, sh);
    const T* xp = reinterpret_cast<const T*>(x.p) + x.co + c;
    const T* g1p = reinterpret_cast<const T*>(gi.g1.p) + gi.g1.co + c;
    const T* g2p = reinterpret_cast<const T*>(gi.g2.p) + gi.g2.co + c;
    T* dp = reinterpret_cast<T*>(dx.p) + dx.co + c;
    const unsigned xs = x.ps, g1s = gi.g1.ps, g2s = gi.g2.ps, ds = dx.ps;
    auto ld = [&](unsigned q, In& in) {
      Vec16<T>::load(xp + q * xs, in.v);
      if (gi.has1) Vec16<T>::load(g1p + q * g1s, in.g1);
      if (gi.has2) Vec16<T>::load(g2p + q * g2s, in.g2);
    };
    auto put = [&](unsigned q, const In& in) {
      float d[N];
      dx_of(in, sc, sh, nullptr, d);
      Vec16<T>::store(dp + q * ds, d);
    };
    for (; pix + pstep < Pu; pix += 2 * pstep) {  // both pixels' loads in flight before either is used
      In a, b;
      ld(pix, a);
      ld(pix + pstep, b);
      put(pix, a);
      put(pix + pstep, b);
    }
    if (pix < Pu) {
      In a;
      ld(pix, a);
      put(pix, a);
    }
  } else {
    const long long total = P * CG;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const typename M::Key key = mask.key();
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
      const int c = N * (int)(idx % CG);
      int b, yy, xx;
      pix_bxy(pd, idx / CG, b, yy, xx);
      In in;
      float sc[N], sh[N], m[N], d[N];
      Vec16<T>::load(vptr<T>(x, b, yy, xx, c), in.v);
      if (M::ON || gi.has1) Vec16<T>::load(vptr<T>(gi.g1, b, yy, xx, c), in.g1);
      if (gi.has2) Vec16<T>::load(vptr<T>(gi.g2, b, yy, xx, c), in.g2);
      ldc<N>(scale + c, sc); ldc<N>(shift + c, sh);
      if constexpr (M::ON) mask.template factor<N>(key, mask.index(C, b, yy, xx, c), m);
      dx_of(in, sc, sh, m, d);
      Vec16<T>::store(reinterpret_cast<T*>(dx.p) + vidx(dx, b, yy, xx, c), d);
    }
  }
}

// rstd_run = 1 / sqrt(running_var + eps), as bn_eval_table_kernel forms it inside scale
__global__ void bn_running_rstd_kernel(int C, const float* rvar, float eps, float* rstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  rstd[c] = 1.f / sqrtf(rvar[c] + eps);
}

// keep (1) / drop (0) of every element of the full extent [B][H][W][C], 4 channels (one Philox call) per thread
__global__ void __launch_bounds__(256) dropout_mask_kernel(DropDev drop, long long quads, unsigned char* out) {
  const DropKey k = drop_key(drop);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
    unsigned keep[4];
    drop_keep4(drop, k, (unsigned long long)q * 4, keep);
    *reinterpret_cast<unsigned*>(out + q * 4) = keep[0] | (keep[1] << 8) | (keep[2] << 16) | (keep[3] << 24);
  }
}

// one call's counter: call = {seed, offset}, then offset += 1 (a single lane; ordered by the stream)
__global__ void dropout_next_kernel(long long* state, long long* call) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const long long seed = state[0], off = state[1];
    call[0] = seed;
    call[1] = off;
    state[1] = off + 1;
  }
}

}  // namespace stc

using namespace stc;

extern "C" int stc_chan_stats_chunks(int B, int H, int W) { return stat_chunks((long long)B * H * W); }

// pixel-dense view: rows and images follow each other without gaps, so pixel p sits at p * ps
static bool pix_dense(const stc_view& v) { return v.rs == (int64_t)v.W * v.ps && v.bs == (int64_t)v.H * v.rs; }

// the streaming (DENSE) element-wise form: pixel-dense views whose element offsets fit 32 bits, and a
// channel-group count dividing 256 (the grid stride is then a whole number of pixels)
static bool stream_ok(int B, const stc_view& v, int C, int N) {
  if (!v.p) return true;
  const long long extent = (long long)B * v.H * v.W * v.ps + v.co + C;
  return pix_dense(v) && extent < (1ll << 31) && 256 % (C / N) == 0;
}
static int grid_stream(long long work) {  // >= 4 pixel-vectors per thread, at most 8 blocks per CU
  return (int)std::max<long long>(1, std::min<long long>((work + 1023) / 1024, 2048));
}

static bool vec_ok(int dtype, int C, const stc_view& v) {
  const int N = dtype == STC_F32 ? 4 : 8;
  return C % N == 0 && C / N <= 256 && v.cs == 1 && v.co % N == 0 && v.ps % N == 0 && v.rs % N == 0 && v.bs % N == 0;
}

// what every entry point derives from (dtype, B, x, C): x's device view, its pixel divider, the pixel count and
// the number of 16-byte channel vectors of all pixels
struct Pixels {
  View v;
  PixDiv pd;
  long long P, work;
};
static Pixels pixels_of(int dtype, int B, const stc_view& x, int C) {
  const long long P = (long long)B * x.H * x.W;
  return Pixels{mkview(x), mkpix(B, x.H, x.W), P, P * (C / (dtype == STC_F32 ? 4 : 8))};
}

extern "C" int stc_chan_stats(int dtype, int B, stc_view x, int C, float* part, int nchunks, void* stream) {
  STC_REQUIRE(vec_ok(dtype, C, x), "stc_chan_stats: C=%d / view not 16-byte vectorisable (NHWC, <= 256 vectors)", C);
  const Pixels s = pixels_of(dtype, B, x, C);
  STC_DT(dtype, hipLaunchKernelGGL(chan_stats_kernel<T_>, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, s.v, s.pd, s.P, C, part, nchunks));
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_bn_apply(int dtype, int B, stc_view x, int C, const float* scale, const float* shift, stc_view y1,
                            float slope1, stc_view y2, float slope2, void* stream) {
  STC_REQUIRE((scale == nullptr) == (shift == nullptr), "stc_bn_apply: scale/shift must come together");
  STC_REQUIRE(y1.p && vec_ok(dtype, C, x) && vec_ok(dtype, C, y1) && (!y2.p || vec_ok(dtype, C, y2)),
              "stc_bn_apply: C=%d / views not 16-byte vectorisable NHWC", C);
  hipStream_t st = (hipStream_t)stream;
  const Pixels s = pixels_of(dtype, B, x, C);
  View o1 = mkview(y1), o2 = y2.p ? mkview(y2) : mkview(y1);
  const int N = dtype == STC_F32 ? 4 : 8;
  const bool dense = stream_ok(B, x, C, N) && stream_ok(B, y1, C, N) && stream_ok(B, y2, C, N);
  const int blocks = dense ? grid_stream(s.work) : grid_for(s.work);
  const int h2 = y2.p != nullptr ? 1 : 0;
#define STC_BA(D_) STC_DT(dtype, hipLaunchKernelGGL((bn_apply_kernel<T_, D_>), dim3(blocks), dim3(256), 0, st, s.v, s.pd, s.P, C, scale, shift, o1, slope1, o2, slope2, h2))
  if (dense) STC_BA(true); else STC_BA(false);
#undef STC_BA
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_chan_sum(int dtype, int B, stc_view x, int C, int Cout, float* part, int nchunks, float* out,
                            void* stream) {
  STC_REQUIRE(vec_ok(dtype, C, x) && Cout <= C, "stc_chan_sum: bad C=%d / view", C);
  hipStream_t st = (hipStream_t)stream;
  const Pixels s = pixels_of(dtype, B, x, C);
  STC_DT(dtype, hipLaunchKernelGGL(chan_sum_kernel<T_>, dim3(nchunks), dim3(256), 0, st, s.v, s.pd, s.P, C, part, nchunks));
  STC_CHECK_LAUNCH();
  hipLaunchKernelGGL(chan_sum_final_kernel, dim3(C), dim3(256), 0, st, (const float*)part, nchunks, C, Cout, out);
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_bn_finalize(const float* part, int nchunks, int C, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, int64_t* num_batches_tracked,
                               float momentum, float eps, float* mean, float* rstd, float* scale, float* shift,
                               void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (part == nullptr) {
    STC_REQUIRE(gamma && beta && running_mean && running_var, "stc_bn_finalize(eval): missing tensors");
    hipLaunchKernelGGL(bn_eval_table_kernel, dim3((C + 255) / 256), dim3(256), 0, st, C, gamma, beta, running_mean,
                       running_var, eps, scale, shift);
  } else {
#define STC_BF(R_) hipLaunchKernelGGL(bn_finalize_kernel<R_>, merge_grid<R_>(C), dim3(256), 0, st, part, nchunks, C, gamma, beta, running_mean, running_var, (long long*)num_batches_tracked, momentum, eps, mean, rstd, scale, shift)
    // up to 4 load groups per lane in registers; more chunks: a block per channel
    if (nchunks <= 1024) STC_BF(WaveMerge); else STC_BF(BlockMerge);
#undef STC_BF
  }
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_bn_bwd_reduce(int dtype, int B, stc_view x, int C, const float* scale, const float* shift,
                                 const float* mean, const float* rstd, stc_view g1, float slope1, stc_view g2,
                                 float slope2, float* part2, int nchunks, void* stream) {
  STC_REQUIRE(vec_ok(dtype, C, x) && (!g1.p || vec_ok(dtype, C, g1)) && (!g2.p || vec_ok(dtype, C, g2)),
              "stc_bn_bwd_reduce: bad C=%d / views", C);
  STC_REQUIRE(scale && shift && mean && rstd, "stc_bn_bwd_reduce: BN tables required");
  GradIn gi = mkgrad(g1, slope1, g2, slope2);
  const Pixels s = pixels_of(dtype, B, x, C);
  STC_DT(dtype, hipLaunchKernelGGL((bn_bwd_reduce_kernel<T_, NoMask>), dim3(nchunks), dim3(256), 0, (hipStream_t)stream, s.v, s.pd, s.P, C, scale, shift, mean, rstd, gi, part2, nchunks, NoMask{}));
  STC_CHECK_LAUNCH();
  return 0;
}

// dgamma / dbeta from the backward reduce's partials: a wave per channel while a lane's one load group covers
// the chunks, else a block per channel
static void bwd_finalize(const float* part2, int nchunks, int C, float* dgamma, float* dbeta, hipStream_t st) {
  if (nchunks <= 256)
    hipLaunchKernelGGL(bn_bwd_finalize_kernel<WaveMerge>, merge_grid<WaveMerge>(C), dim3(256), 0, st, part2, nchunks, C, dgamma, dbeta);
  else
    hipLaunchKernelGGL(bn_bwd_finalize_kernel<BlockMerge>, merge_grid<BlockMerge>(C), dim3(256), 0, st, part2, nchunks, C, dgamma, dbeta);
}

extern "C" int stc_bn_bwd_apply(int dtype, int B, stc_view x, int C, const float* scale, const float* shift,
                                const float* mean, const float* rstd, const float* gamma, stc_view g1, float slope1,
                                stc_view g2, float slope2, const float* part2, int nchunks, stc_view dx,
                                float* dgamma, float* dbeta, void* stream) {
  STC_REQUIRE(vec_ok(dtype, C, x) && vec_ok(dtype, C, dx) && (!g1.p || vec_ok(dtype, C, g1)) &&
                  (!g2.p || vec_ok(dtype, C, g2)),
              "stc_bn_bwd_apply: bad C=%d / views", C);
  hipStream_t st = (hipStream_t)stream;
  GradIn gi = mkgrad(g1, slope1, g2, slope2);
  if (mean) {
    STC_REQUIRE(part2 && dgamma && dbeta && gamma && rstd && scale && shift, "stc_bn_bwd_apply: missing BN tensors");
    bwd_finalize(part2, nchunks, C, dgamma, dbeta, st);
    STC_CHECK_LAUNCH();
  }
  const Pixels s = pixels_of(dtype, B, x, C);
  View o = mkview(dx);
  const int N = dtype == STC_F32 ? 4 : 8;
  const bool dense = stream_ok(B, x, C, N) && stream_ok(B, dx, C, N) && stream_ok(B, g1, C, N) && stream_ok(B, g2, C, N);
  const int blocks = dense ? grid_stream(s.work) : grid_for(s.work);
#define STC_BB(D_) STC_DT(dtype, hipLaunchKernelGGL((bn_bwd_apply_kernel<T_, D_>), dim3(blocks), dim3(256), 0, st, s.v, s.pd, s.P, C, scale, shift, mean, rstd, gamma, gi, dgamma, dbeta, o))
  if (dense) STC_BB(true); else STC_BB(false);
#undef STC_BB
  STC_CHECK_LAUNCH();
  return 0;
}

// ---- dropout (use_dropout=True generators): philox.hpp holds the mask function
static int mkdrop(const stc_dropout* d, int B, int C, DropDev* out, const char* who) {
  STC_REQUIRE(d && d->state, "%s: dropout block with a device {seed, offset} required", who);
  STC_REQUIRE(d->p >= 0.0 && d->p < 1.0, "%s: drop probability %g outside [0, 1)", who, d->p);
  STC_REQUIRE(d->level >= 0 && d->H > 0 && d->W > 0 && B > 0 && C > 0 && C % 4 == 0,
              "%s: bad dropout level %d / extent %d x %d x %d x %d (C %% 4 == 0)", who, d->level, B, d->H, d->W, C);
  STC_REQUIRE((long long)B * d->H * d->W * C < (1ll << 34), "%s: more than 2^34 elements under one dropout level", who);
  out->state = reinterpret_cast<const unsigned long long*>(d->state);
  out->level = (unsigned)d->level;
  out->thresh = (unsigned)(unsigned long long)(d->p * 4294967296.0);  // floor(p * 2^32)
  out->scale = (float)(1.0 / (1.0 - d->p));
  out->H = d->H; out->W = d->W;
  return 0;
}

extern "C" int stc_dropout_next(int64_t* state, int64_t* call_state, void* stream) {
  STC_REQUIRE(state && call_state, "stc_dropout_next: state and call_state required");
  hipLaunchKernelGGL(dropout_next_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)state,
                     (long long*)call_state);
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_dropout_mask(const stc_dropout* drop, int B, int C, uint8_t* out, void* stream) {
  DropDev dd;
  if (int rc = mkdrop(drop, B, C, &dd, "stc_dropout_mask")) return rc;
  STC_REQUIRE(out, "stc_dropout_mask: output required");
  const long long quads = (long long)B * drop->H * drop->W * C / 4;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for(quads)), dim3(256), 0, (hipStream_t)stream, dd, quads, out);
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_bn_apply_drop(int dtype, int B, stc_view x, int C, const float* scale, const float* shift,
                                 stc_view y1, float slope1, stc_view y2, float slope2, const stc_dropout* drop,
                                 void* stream) {
  STC_REQUIRE((scale == nullptr) == (shift == nullptr), "stc_bn_apply_drop: scale/shift must come together");
  STC_REQUIRE(y1.p && vec_ok(dtype, C, x) && vec_ok(dtype, C, y1) && (!y2.p || vec_ok(dtype, C, y2)),
              "stc_bn_apply_drop: C=%d / views not 16-byte vectorisable NHWC", C);
  PhiloxMask mask;
  if (int rc = mkdrop(drop, B, C, &mask.d, "stc_bn_apply_drop")) return rc;
  STC_REQUIRE(x.H <= drop->H && x.W <= drop->W, "stc_bn_apply_drop: view %d x %d outside the dropout extent %d x %d",
              x.H, x.W, drop->H, drop->W);
  const Pixels s = pixels_of(dtype, B, x, C);
  View o1 = mkview(y1), o2 = y2.p ? mkview(y2) : mkview(y1);
  const int blocks = grid_for(s.work);  // covers the tensor once at the generator's sizes (launch-latency bound)
  const int h2 = y2.p != nullptr ? 1 : 0;
  STC_DT(dtype, hipLaunchKernelGGL(bn_apply_drop_kernel<T_>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, s.v, s.pd, s.P, C, scale, shift, o1, slope1, o2, slope2, h2, mask));
  STC_CHECK_LAUNCH();
  return 0;
}

// stc_conv_bn_fwd with the dropout-aware apply: the same three launches from one call
extern "C" int stc_conv_bn_fwd_drop(int dtype, int kind, int B, stc_view x, int Cin, const void* w_packed, int Cout,
                                    stc_view y, float* fws, int nchunks, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                    float momentum, float eps, stc_view apply_x, stc_view y1, float slope1,
                                    stc_view y2, float slope2, const stc_dropout* drop, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  STC_REQUIRE(fws && nchunks > 0 && gamma && beta, "stc_conv_bn_fwd_drop: statistics workspace and BN affine required");
  STC_REQUIRE(y1.p, "stc_conv_bn_fwd_drop: an apply output is required");
  DropDev dd;
  if (int rc = mkdrop(drop, B, Cout, &dd, "stc_conv_bn_fwd_drop")) return rc;  // (before anything is launched)
  // what stc_bn_apply_drop would refuse, also before the conv and the finalize: a refused call leaves the raw
  // output and the running statistics alone
  STC_REQUIRE(vec_ok(dtype, Cout, apply_x) && vec_ok(dtype, Cout, y1) && (!y2.p || vec_ok(dtype, Cout, y2)),
              "stc_conv_bn_fwd_drop: C=%d / activation views not 16-byte vectorisable NHWC", Cout);
  STC_REQUIRE(apply_x.H <= drop->H && apply_x.W <= drop->W,
              "stc_conv_bn_fwd_drop: view %d x %d outside the dropout extent %d x %d", apply_x.H, apply_x.W, drop->H,
              drop->W);
  int rc = stc_conv_fwd_ex(dtype, kind, B, x, Cin, w_packed, Cout, y, nullptr, 0, 0, fws, nchunks, nullptr, workspace,
                           workspace_bytes, stream);
  if (rc) return rc;
  float* tab = fws + (int64_t)nchunks * Cout * 4;
  rc = stc_bn_finalize(fws, nchunks, Cout, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps,
                       tab, tab + Cout, tab + 2 * Cout, tab + 3 * Cout, stream);
  if (rc) return rc;
  return stc_bn_apply_drop(dtype, B, apply_x, Cout, tab + 2 * Cout, tab + 3 * Cout, y1, slope1, y2, slope2, drop,
                           stream);
}

extern "C" int stc_bn_bwd_reduce_drop(int dtype, int B, stc_view x, int C, const float* scale, const float* shift,
                                      const float* mean, const float* rstd, stc_view g1, float slope1, stc_view g2,
                                      float slope2, const stc_dropout* drop, float* part2, int nchunks, void* stream) {
  STC_REQUIRE(vec_ok(dtype, C, x) && g1.p && vec_ok(dtype, C, g1) && (!g2.p || vec_ok(dtype, C, g2)),
              "stc_bn_bwd_reduce_drop: bad C=%d / views (g1 required)", C);
  STC_REQUIRE(scale && shift && mean && rstd, "stc_bn_bwd_reduce_drop: BN tables required");
  PhiloxMask mask;
  if (int rc = mkdrop(drop, B, C, &mask.d, "stc_bn_bwd_reduce_drop")) return rc;
  STC_REQUIRE(x.H <= drop->H && x.W <= drop->W, "stc_bn_bwd_reduce_drop: view outside the dropout extent");
  GradIn gi = mkgrad(g1, slope1, g2, slope2);
  const Pixels s = pixels_of(dtype, B, x, C);
  STC_DT(dtype, hipLaunchKernelGGL((bn_bwd_reduce_kernel<T_, PhiloxMask>), dim3(nchunks), dim3(256), 0, (hipStream_t)stream, s.v, s.pd, s.P, C, scale, shift, mean, rstd, gi, part2, nchunks, mask));
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_bn_bwd_apply_drop(int dtype, int B, stc_view x, int C, const float* scale, const float* shift,
                                     const float* mean, const float* rstd, const float* gamma, stc_view g1,
                                     float slope1, stc_view g2, float slope2, const stc_dropout* drop,
                                     const float* part2, int nchunks, stc_view dx, float* dgamma, float* dbeta,
                                     void* stream) {
  STC_REQUIRE(vec_ok(dtype, C, x) && vec_ok(dtype, C, dx) && g1.p && vec_ok(dtype, C, g1) &&
                  (!g2.p || vec_ok(dtype, C, g2)),
              "stc_bn_bwd_apply_drop: bad C=%d / views (g1 required)", C);
  STC_REQUIRE(mean && part2 && nchunks > 0 && dgamma && dbeta && gamma && rstd && scale && shift,
              "stc_bn_bwd_apply_drop: missing BN tensors");
  PhiloxMask mask;
  if (int rc = mkdrop(drop, B, C, &mask.d, "stc_bn_bwd_apply_drop")) return rc;
  STC_REQUIRE(x.H <= drop->H && x.W <= drop->W, "stc_bn_bwd_apply_drop: view outside the dropout extent");
  hipStream_t st = (hipStream_t)stream;
  GradIn gi = mkgrad(g1, slope1, g2, slope2);
  bwd_finalize(part2, nchunks, C, dgamma, dbeta, st);
  STC_CHECK_LAUNCH();
  const Pixels s = pixels_of(dtype, B, x, C);
  View o = mkview(dx);
  STC_DT(dtype, hipLaunchKernelGGL(bn_bwd_apply_drop_kernel<T_>, dim3(grid_for(s.work)), dim3(256), 0, st, s.v, s.pd, s.P, C, scale, shift, mean, rstd, gamma, gi, dgamma, dbeta, o, mask));
  STC_CHECK_LAUNCH();
  return 0;
}

// ---- frozen statistics (a BatchNorm layer that normalises with its running statistics)
extern "C" int stc_bn_running_rstd(int C, const float* running_var, float eps, float* rstd, void* stream) {
  STC_REQUIRE(C > 0 && running_var && rstd, "stc_bn_running_rstd: running_var and an output of C > 0 floats required");
  hipLaunchKernelGGL(bn_running_rstd_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, C, running_var,
                     eps, rstd);
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_bn_bwd_frozen(int dtype, int B, stc_view x, int C, const float* scale, const float* shift,
                                 const float* mean, const float* rstd, stc_view g1, float slope1, stc_view g2,
                                 float slope2, const stc_dropout* drop, float* part, int nchunks, stc_view dx,
                                 float* dgamma, float* dbeta, void* stream) {
  STC_REQUIRE(vec_ok(dtype, C, x) && dx.p && vec_ok(dtype, C, dx) && (!g1.p || vec_ok(dtype, C, g1)) &&
                  (!g2.p || vec_ok(dtype, C, g2)),
              "stc_bn_bwd_frozen: bad C=%d / views", C);
  STC_REQUIRE(scale && shift, "stc_bn_bwd_frozen: the scale / shift table is required");
  STC_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "stc_bn_bwd_frozen: dgamma / dbeta must come together");
  const bool sums = dgamma != nullptr;
  const Pixels s = pixels_of(dtype, B, x, C);
  if (sums) {
    STC_REQUIRE(mean && rstd && part, "stc_bn_bwd_frozen: running mean / rstd tables and a partials buffer required");
    STC_REQUIRE(nchunks == stat_chunks(s.P), "stc_bn_bwd_frozen: nchunks=%d, not the %d chunks of %lld pixels",
                nchunks, stat_chunks(s.P), s.P);
  }
  PhiloxMask mask;
  if (drop) {
    STC_REQUIRE(g1.p, "stc_bn_bwd_frozen: a dropout block needs g1, the gradient that passes through it");
    if (int rc = mkdrop(drop, B, C, &mask.d, "stc_bn_bwd_frozen")) return rc;
    STC_REQUIRE(x.H <= drop->H && x.W <= drop->W, "stc_bn_bwd_frozen: view outside the dropout extent");
  }
  hipStream_t st = (hipStream_t)stream;
  GradIn gi = mkgrad(g1, slope1, g2, slope2);
  View o = mkview(dx);
  if (sums) {
    if (drop) STC_DT(dtype, hipLaunchKernelGGL((bn_bwd_frozen_sums_kernel<T_, PhiloxMask>), dim3(nchunks), dim3(256), 0, st, s.v, s.pd, s.P, C, scale, shift, mean, rstd, gi, part, nchunks, o, mask));
    else STC_DT(dtype, hipLaunchKernelGGL((bn_bwd_frozen_sums_kernel<T_, NoMask>), dim3(nchunks), dim3(256), 0, st, s.v, s.pd, s.P, C, scale, shift, mean, rstd, gi, part, nchunks, o, NoMask{}));
    STC_CHECK_LAUNCH();
    bwd_finalize(part, nchunks, C, dgamma, dbeta, st);
    STC_CHECK_LAUNCH();
    return 0;
  }
  const int N = dtype == STC_F32 ? 4 : 8;
  const bool dense = !drop && stream_ok(B, x, C, N) && stream_ok(B, dx, C, N) && stream_ok(B, g1, C, N) && stream_ok(B, g2, C, N);
  const int blocks = dense ? grid_stream(s.work) : grid_for(s.work);
#define STC_FZ(D_, M_, m_) STC_DT(dtype, hipLaunchKernelGGL((bn_bwd_frozen_kernel<T_, D_, M_>), dim3(blocks), dim3(256), 0, st, s.v, s.pd, s.P, C, scale, shift, gi, o, m_))
  if (dense) STC_FZ(true, NoMask, NoMask{});
  else if (drop) STC_FZ(false, PhiloxMask, mask);
  else STC_FZ(false, NoMask, NoMask{});
#undef STC_FZ
  STC_CHECK_LAUNCH();
  return 0;
}

// ---- sync statistics (nn.SyncBatchNorm: batch statistics over all data-parallel ranks)
extern "C" int stc_bn_stats_pack(const float* part, int nchunks, int C, float* rec, void* stream) {
  STC_REQUIRE(part && rec && nchunks > 0 && C > 0, "stc_bn_stats_pack: partials of nchunks > 0 chunks, C > 0 and a record buffer required");
  hipStream_t st = (hipStream_t)stream;
  // (the lane policies of stc_bn_finalize)
  if (nchunks <= 1024) hipLaunchKernelGGL(bn_stats_pack_kernel<WaveMerge>, merge_grid<WaveMerge>(C), dim3(256), 0, st, part, nchunks, C, rec);
  else hipLaunchKernelGGL(bn_stats_pack_kernel<BlockMerge>, merge_grid<BlockMerge>(C), dim3(256), 0, st, part, nchunks, C, rec);
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_bn_bwd_sums(const float* part2, int nchunks, int C, float* dgamma, float* dbeta, float* rec,
                               void* stream) {
  STC_REQUIRE(part2 && rec && nchunks > 0 && C > 0, "stc_bn_bwd_sums: partials of nchunks > 0 chunks, C > 0 and a record buffer required");
  STC_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "stc_bn_bwd_sums: dgamma / dbeta must come together");
  hipStream_t st = (hipStream_t)stream;
  // (the lane policies of bwd_finalize)
  if (nchunks <= 256) hipLaunchKernelGGL(bn_bwd_sums_kernel<WaveMerge>, merge_grid<WaveMerge>(C), dim3(256), 0, st, part2, nchunks, C, dgamma, dbeta, rec);
  else hipLaunchKernelGGL(bn_bwd_sums_kernel<BlockMerge>, merge_grid<BlockMerge>(C), dim3(256), 0, st, part2, nchunks, C, dgamma, dbeta, rec);
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_bn_bwd_apply_sync(int dtype, int B, stc_view x, int C, const float* scale, const float* shift,
                                     const float* mean, const float* rstd, const float* gamma, stc_view g1,
                                     float slope1, stc_view g2, float slope2, const stc_dropout* drop,
                                     const float* recs, int world, int64_t count, stc_view dx, void* stream) {
  STC_REQUIRE(vec_ok(dtype, C, x) && dx.p && vec_ok(dtype, C, dx) && (!g1.p || vec_ok(dtype, C, g1)) &&
                  (!g2.p || vec_ok(dtype, C, g2)),
              "stc_bn_bwd_apply_sync: bad C=%d / views", C);
  STC_REQUIRE(mean && rstd && gamma && scale && shift && recs, "stc_bn_bwd_apply_sync: missing BN tensors / records");
  const Pixels s = pixels_of(dtype, B, x, C);
  STC_REQUIRE(world >= 1 && count >= s.P, "stc_bn_bwd_apply_sync: world=%d, count=%lld: at least one rank and at least this rank's %lld pixels",
              world, (long long)count, s.P);
  PhiloxMask mask;
  if (drop) {
    STC_REQUIRE(g1.p, "stc_bn_bwd_apply_sync: a dropout block needs g1, the gradient that passes through it");
    if (int rc = mkdrop(drop, B, C, &mask.d, "stc_bn_bwd_apply_sync")) return rc;
    STC_REQUIRE(x.H <= drop->H && x.W <= drop->W, "stc_bn_bwd_apply_sync: view outside the dropout extent");
  }
  hipStream_t st = (hipStream_t)stream;
  GradIn gi = mkgrad(g1, slope1, g2, slope2);
  View o = mkview(dx);
  const int blocks = grid_for(s.work);
  if (drop) STC_DT(dtype, hipLaunchKernelGGL((bn_bwd_apply_sync_kernel<T_, PhiloxMask>), dim3(blocks), dim3(256), 0, st, s.v, s.pd, s.P, C, scale, shift, mean, rstd, gamma, gi, recs, world, (long long)count, o, mask));
  else STC_DT(dtype, hipLaunchKernelGGL((bn_bwd_apply_sync_kernel<T_, NoMask>), dim3(blocks), dim3(256), 0, st, s.v, s.pd, s.P, C, scale, shift, mean, rstd, gamma, gi, recs, world, (long long)count, o, NoMask{}));
  STC_CHECK_LAUNCH();
  return 0;
}
