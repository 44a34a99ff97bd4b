// InstanceNorm2d forward / backward fused with LeakyReLU / ReLU
// (STCGAN/networks.py:107,109,170,179 with norm_layer=nn.InstanceNorm2d).
//
// Statistics are per (sample, channel) over one H x W plane, from 128x128 planes of 64 channels
// down to 2x2 planes of 512, so the work is split by plane size (stc_in_plan):
//   tiny      P <= TINY_MAX pixels: a thread owns one (sample, channel vector), holds the plane in
//             registers and does statistics + apply (or reduce + dx) alone: one launch, no cross-lane step.
//   resident  a workgroup owns one (sample, channel slab) whose plane fits its registers (KV vectors
//             per thread): the plane is read once; shifted mean, centred variance and apply in one
//             launch, the backward likewise.
//   streamed  the plane is cut into pixel chunks of that size: the first launch writes per-chunk
//             {mean, centred M2} (or {sum dn, sum dn*xhat}) to the workspace, the second merges its own
//             (sample, slab) partials in chunk order and applies; its chunk 0 writes mean / rstd.
// Thread layout of a workgroup: tid = pl * SV + cgl, cgl the channel vector inside the slab of SV
// vectors (SV * 16 bytes contiguous per pixel), pl the pixel lane; lane pl holds pixels p0 + pl + j*RL.
// Every sum is a fixed-order chain (a thread's own pixels in order, then the pixel lanes -- a wave
// butterfly and the wave totals in order when SV divides the wave, else a halving tree in LDS --
// then the chunks in order): bitwise reproducible, no atomics.  The variance is
// always the centred sum of (x - mean)^2 around the chunk's own mean (Chan's merge across chunks, fp64),
// never E[x^2] - E[x]^2.
#include <algorithm>

#include "common.hpp"
#include "vec16.hpp"

namespace stc {
namespace inorm {

constexpr int TINY_MAX = 8;   // pixels of a plane one thread keeps in registers (4x4 measured faster as resident)
constexpr int TINY_NT = 64;   // threads per tiny workgroup (one wave: the backward keeps x and an fp32 dn plane in registers)
constexpr int NT = 512;       // threads per resident / streamed workgroup
constexpr int KV = 8;         // 16-byte vectors per thread (x; the backward also g1 and g2)
#ifndef STC_IN_SLAB_VECS
#define STC_IN_SLAB_VECS 8  // channel vectors per slab: 8 x 16 bytes = one 128-byte line per pixel
#endif
constexpr int SV_MAX = STC_IN_SLAB_VECS;

template <typename T>
__device__ __forceinline__ uint4 ldv(const View& v, int b, int y, int x, int c) {
  return Vec16<T>::ldraw(reinterpret_cast<const T*>(v.p) + vidx(v, b, y, x, c));
}
template <typename T>
__device__ __forceinline__ void stv(const View& v, int b, int y, int x, int c, const uint4& u) {
  Vec16<T>::straw(reinterpret_cast<T*>(v.p) + vidx(v, b, y, x, c), u);
}
template <int N>
__device__ __forceinline__ void affine_of(const float* gamma, const float* beta, int c, float* ga, float* be) {
  if (gamma) { ldc<N>(gamma + c, ga); ldc<N>(beta + c, be); }
  else {
#pragma unroll
    for (int e = 0; e < N; ++e) { ga[e] = 1.f; be[e] = 0.f; }
  }
}
__device__ __forceinline__ float rstd_of(float var, float eps) { return (float)(1.0 / sqrt((double)var + (double)eps)); }

struct Geo {
  int W, P, C, CG;      // plane width, pixels per plane, channels, channel vectors
  int SV, RL, rl2;      // vectors per slab, pixel lanes per workgroup, smallest power of two >= RL
  int shfl;             // SV divides the wave: the lanes of a channel vector sit SV apart inside every wave
  int pc, nchunks;      // pixels per chunk, chunks per sample
};
struct Outs {
  View y1, y2;
  float s1, s2;
  int has2, Ha, Wa;  // outputs cover the top-left Ha x Wa of the statistics extent
};
struct Grads {
  View g1, g2;
  float s1, s2;
  int has1, has2;
};

// v[e] <- sum over the pixel lanes of the same channel vector, in a fixed halving-tree order; every
// thread of the workgroup calls it (idle ones with zeros) and gets its channel vector's totals back
template <int NF>
__device__ __forceinline__ void lane_tree(float* v, float* red, const Geo& g, int pl) {
  const int tid = threadIdx.x;
  if (g.shfl) {
    // a butterfly over the wave's pixel lanes (both partners form the same sum), then the waves' totals in wave
    // order: two barriers instead of one per tree level
    for (int o = 32; o >= g.SV; o >>= 1) {
#pragma unroll
      for (int e = 0; e < NF; ++e) v[e] += __shfl_xor(v[e], o, 64);
    }
    const int lane = tid & 63, wave = tid >> 6, cgl = lane % g.SV;
    if (lane < g.SV) {
#pragma unroll
      for (int e = 0; e < NF; ++e) red[(wave * g.SV + lane) * NF + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < NF; ++e) v[e] = 0.f;
#pragma unroll 1
    for (int w = 0; w < NT / 64; ++w) {  // (not unrolled: NF * 8 loads in flight would spill the backward)
#pragma unroll
      for (int e = 0; e < NF; ++e) v[e] += red[(w * g.SV + cgl) * NF + e];
    }
    __syncthreads();
    return;
  }
#pragma unroll
  for (int e = 0; e < NF; ++e) red[tid * NF + e] = v[e];
  __syncthreads();
  for (int s = g.rl2 >> 1; s >= 1; s >>= 1) {
    if (pl < s && pl + s < g.RL) {
#pragma unroll
      for (int e = 0; e < NF; ++e) red[tid * NF + e] += red[(tid + s * g.SV) * NF + e];
    }
    __syncthreads();
  }
  const int cgl = tid % g.SV;
#pragma unroll
  for (int e = 0; e < NF; ++e) v[e] = red[cgl * NF + e];
  __syncthreads();
}

template <typename T, int N>
__device__ __forceinline__ void emit(const Outs& o, int b, int y, int x, int c, const float* f, const float* mu,
                                     const float* rs, const float* ga, const float* be) {
  float n[N], r[N];
#pragma unroll
  for (int e = 0; e < N; ++e) n[e] = fmaf((f[e] - mu[e]) * rs[e], ga[e], be[e]);
#pragma unroll
  for (int e = 0; e < N; ++e) r[e] = act(n[e], o.s1);
  stv<T>(o.y1, b, y, x, c, Vec16<T>::pack(r));
  if (o.has2) {
#pragma unroll
    for (int e = 0; e < N; ++e) r[e] = act(n[e], o.s2);
    stv<T>(o.y2, b, y, x, c, Vec16<T>::pack(r));
  }
}

// dn = g1*act1'(n) + g2*act2'(n) and xhat of one vector; n is formed exactly as the forward forms it
template <typename T, int N>
__device__ __forceinline__ void dn_xhat(const Grads& gr, const uint4& xr, const uint4& ar, const uint4& br,
                                        const float* mu, const float* rs, const float* ga, const float* be, float* dn,
                                        float* xh) {
  float f[N], a[N], q[N];
  Vec16<T>::unpack(xr, f);
  Vec16<T>::unpack(ar, a);
  Vec16<T>::unpack(br, q);
#pragma unroll
  for (int e = 0; e < N; ++e) {
    xh[e] = (f[e] - mu[e]) * rs[e];
    const float n = fmaf(xh[e], ga[e], be[e]);
    float d = 0.f;
    if (gr.has1) d += a[e] * dact(n, gr.s1);
    if (gr.has2) d += q[e] * dact(n, gr.s2);
    dn[e] = d;
  }
}

// ---------------------------------------------------------------- tiny: one thread per (sample, channel vector)
template <typename T>
__global__ void __launch_bounds__(TINY_NT) in_fwd_tiny_kernel(View x, Geo g, int B, const float* gamma, const float* beta,
                                                              float eps, float* mean, float* rstd, Outs o) {
  constexpr int N = Vec16<T>::N;
  const long long t = (long long)blockIdx.x * TINY_NT + threadIdx.x;
  if (t >= (long long)B * g.CG) return;
  const int b = (int)(t / g.CG), c = N * (int)(t % g.CG);
  uint4 r[TINY_MAX];
#pragma unroll
  for (int j = 0; j < TINY_MAX; ++j)
    if (j < g.P) r[j] = ldv<T>(x, b, j / g.W, j % g.W, c);
  float sh[N], s[N], mu[N], q[N], rs[N], ga[N], be[N];
  Vec16<T>::unpack(r[0], sh);
#pragma unroll
  for (int e = 0; e < N; ++e) { s[e] = 0.f; q[e] = 0.f; }
#pragma unroll
  for (int j = 0; j < TINY_MAX; ++j)
    if (j < g.P) {
      float f[N];
      Vec16<T>::unpack(r[j], f);
#pragma unroll
      for (int e = 0; e < N; ++e) s[e] += f[e] - sh[e];
    }
#pragma unroll
  for (int e = 0; e < N; ++e) mu[e] = sh[e] + s[e] / (float)g.P;
#pragma unroll
  for (int j = 0; j < TINY_MAX; ++j)
    if (j < g.P) {
      float f[N];
      Vec16<T>::unpack(r[j], f);
#pragma unroll
      for (int e = 0; e < N; ++e) { const float d = f[e] - mu[e]; q[e] = fmaf(d, d, q[e]); }
    }
#pragma unroll
  for (int e = 0; e < N; ++e) {
    rs[e] = rstd_of(q[e] / (float)g.P, eps);
    mean[(long long)b * g.C + c + e] = mu[e];
    rstd[(long long)b * g.C + c + e] = rs[e];
  }
  affine_of<N>(gamma, beta, c, ga, be);
#pragma unroll
  for (int j = 0; j < TINY_MAX; ++j)
    if (j < g.P) {
      const int y = j / g.W, xx = j % g.W;
      if (y < o.Ha && xx < o.Wa) {
        float f[N];
        Vec16<T>::unpack(r[j], f);
        emit<T, N>(o, b, y, xx, c, f, mu, rs, ga, be);
      }
    }
}

template <typename T>
__global__ void __launch_bounds__(TINY_NT) in_bwd_tiny_kernel(View x, Geo g, int B, const float* gamma, const float* beta,
                                                              const float* mean, const float* rstd, Grads gr, View dx,
                                                              float* sums) {
  constexpr int N = Vec16<T>::N;
  const long long t = (long long)blockIdx.x * TINY_NT + threadIdx.x;
  if (t >= (long long)B * g.CG) return;
  const int b = (int)(t / g.CG), c = N * (int)(t % g.CG);
  float mu[N], rs[N], ga[N], be[N], A[N], Bs[N];
  ldc<N>(mean + (long long)b * g.C + c, mu);
  ldc<N>(rstd + (long long)b * g.C + c, rs);
  affine_of<N>(gamma, beta, c, ga, be);
#pragma unroll
  for (int e = 0; e < N; ++e) { A[e] = 0.f; Bs[e] = 0.f; }
  // the plane stays in registers as raw x and fp32 dn (xhat is one subtract and one multiply away from x)
  uint4 r[TINY_MAX];
  float dnr[TINY_MAX][N];
#pragma unroll
  for (int j = 0; j < TINY_MAX; ++j)
    if (j < g.P) {
      const int y = j / g.W, xx = j % g.W;
      r[j] = ldv<T>(x, b, y, xx, c);
      uint4 a = make_uint4(0, 0, 0, 0), q = a;
      if (gr.has1) a = ldv<T>(gr.g1, b, y, xx, c);
      if (gr.has2) q = ldv<T>(gr.g2, b, y, xx, c);
      float xh[N];
      dn_xhat<T, N>(gr, r[j], a, q, mu, rs, ga, be, dnr[j], xh);
#pragma unroll
      for (int e = 0; e < N; ++e) { A[e] += dnr[j][e]; Bs[e] = fmaf(dnr[j][e], xh[e], Bs[e]); }
    }
  if (sums) {
#pragma unroll
    for (int e = 0; e < N; ++e)
      *reinterpret_cast<float2*>(sums + ((long long)b * g.C + c + e) * 2) = make_float2(A[e], Bs[e]);
  }
  float k[N];
#pragma unroll
  for (int e = 0; e < N; ++e) { k[e] = ga[e] * rs[e]; A[e] = A[e] / (float)g.P; Bs[e] = Bs[e] / (float)g.P; }
#pragma unroll
  for (int j = 0; j < TINY_MAX; ++j)
    if (j < g.P) {
      float f[N], d[N];
      Vec16<T>::unpack(r[j], f);
#pragma unroll
      for (int e = 0; e < N; ++e) d[e] = k[e] * (dnr[j][e] - A[e] - (f[e] - mu[e]) * rs[e] * Bs[e]);
      stv<T>(dx, b, j / g.W, j % g.W, c, Vec16<T>::pack(d));
    }
}

// ---------------------------------------------------------------- resident / streamed
// grid = (chunks, slabs, B).  MODE 0: resident, one launch.  MODE 1: streamed, chunk statistics to
// part[b][chunk][C][2] = {chunk mean, chunk sum (x - chunk mean)^2}.  MODE 2: streamed, merge + apply.
template <typename T, int MODE>
__global__ void __launch_bounds__(NT) in_fwd_kernel(View x, Geo g, const float* gamma, const float* beta, float eps,
                                                    float* mean, float* rstd, Outs o, float* part) {
  constexpr int N = Vec16<T>::N;
  __shared__ float red[NT * N];
  const int tid = threadIdx.x, cgl = tid % g.SV, pl = tid / g.SV;
  const int cg = blockIdx.y * g.SV + cgl, b = blockIdx.z, ch = blockIdx.x;
  const int p0 = ch * g.pc, p1 = min(g.P, p0 + g.pc);
  const bool on = pl < g.RL && cg < g.CG;
  const int c = N * cg;
  uint4 r[KV];
#pragma unroll
  for (int j = 0; j < KV; ++j) {
    const int pix = p0 + pl + j * g.RL;
    if (on && pix < p1) r[j] = ldv<T>(x, b, pix / g.W, pix % g.W, c);
  }
  float mu[N], rs[N];
  if (MODE != 2) {
    float sh[N], s[N], q[N];
#pragma unroll
    for (int e = 0; e < N; ++e) { sh[e] = 0.f; s[e] = 0.f; q[e] = 0.f; }
    if (on) Vec16<T>::unpack(ldv<T>(x, b, p0 / g.W, p0 % g.W, c), sh);  // the chunk's first pixel: the shift
#pragma unroll
    for (int j = 0; j < KV; ++j)
      if (on && p0 + pl + j * g.RL < p1) {
        float f[N];
        Vec16<T>::unpack(r[j], f);
#pragma unroll
        for (int e = 0; e < N; ++e) s[e] += f[e] - sh[e];
      }
    lane_tree<N>(s, red, g, pl);
    const float n = (float)(p1 - p0);
#pragma unroll
    for (int e = 0; e < N; ++e) mu[e] = sh[e] + s[e] / n;
#pragma unroll
    for (int j = 0; j < KV; ++j)
      if (on && p0 + pl + j * g.RL < p1) {
        float f[N];
        Vec16<T>::unpack(r[j], f);
#pragma unroll
        for (int e = 0; e < N; ++e) { const float d = f[e] - mu[e]; q[e] = fmaf(d, d, q[e]); }
      }
    lane_tree<N>(q, red, g, pl);
    if (MODE == 1) {
      if (on && pl == 0) {
#pragma unroll
        for (int e = 0; e < N; ++e)
          *reinterpret_cast<float2*>(part + (((long long)b * g.nchunks + ch) * g.C + c + e) * 2) = make_float2(mu[e], q[e]);
      }
      return;
    }
#pragma unroll
    for (int e = 0; e < N; ++e) rs[e] = rstd_of(q[e] / n, eps);
  } else {
    // this (sample, slab)'s chunks merged in chunk order (Chan, fp64) by the slab's first pixel lane
    if (on && pl == 0) {
      double cnt = 0.0, M[N], M2[N];
#pragma unroll
      for (int e = 0; e < N; ++e) { M[e] = 0.0; M2[e] = 0.0; }
      for (int k = 0; k < g.nchunks; ++k) {
        const double nk = (double)(min(g.P, (k + 1) * g.pc) - k * g.pc);
        const double tot = cnt + nk, w = nk / tot;
        float pv[2 * N];
        ldc<2 * N>(part + (((long long)b * g.nchunks + k) * g.C + c) * 2, pv);
#pragma unroll
        for (int e = 0; e < N; ++e) {
          const double d = (double)pv[2 * e] - M[e];
          M[e] += d * w;
          M2[e] += (double)pv[2 * e + 1] + d * d * cnt * w;
        }
        cnt = tot;
      }
#pragma unroll
      for (int e = 0; e < N; ++e) {
        red[cgl * 2 * N + e] = (float)M[e];
        red[cgl * 2 * N + N + e] = (float)(1.0 / sqrt(M2[e] / cnt + (double)eps));
      }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < N; ++e) { mu[e] = red[cgl * 2 * N + e]; rs[e] = red[cgl * 2 * N + N + e]; }
  }
  if (on && pl == 0 && ch == 0) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
      mean[(long long)b * g.C + c + e] = mu[e];
      rstd[(long long)b * g.C + c + e] = rs[e];
    }
  }
  if (!on) return;
  float ga[N], be[N];
  affine_of<N>(gamma, beta, c, ga, be);
#pragma unroll
  for (int j = 0; j < KV; ++j) {
    const int pix = p0 + pl + j * g.RL;
    if (pix < p1) {
      const int y = pix / g.W, xx = pix % g.W;
      if (y < o.Ha && xx < o.Wa) {
        float f[N];
        Vec16<T>::unpack(r[j], f);
        emit<T, N>(o, b, y, xx, c, f, mu, rs, ga, be);
      }
    }
  }
}

// MODE 0: resident.  MODE 1: streamed, part[b][chunk][C][2] = {sum dn, sum dn*xhat} of the chunk.
// MODE 2: streamed, merge in chunk order + dx.  sums (optional): [B][C][2] plane totals for dgamma / dbeta.
template <typename T, int MODE>
__global__ void __launch_bounds__(NT) in_bwd_kernel(View x, Geo g, const float* gamma, const float* beta,
                                                    const float* mean, const float* rstd, Grads gr, View dx, float* part,
                                                    float* sums) {
  constexpr int N = Vec16<T>::N;
  __shared__ float red[NT * 2 * N];
  const int tid = threadIdx.x, cgl = tid % g.SV, pl = tid / g.SV;
  const int cg = blockIdx.y * g.SV + cgl, b = blockIdx.z, ch = blockIdx.x;
  const int p0 = ch * g.pc, p1 = min(g.P, p0 + g.pc);
  const bool on = pl < g.RL && cg < g.CG;
  const int c = N * cg;
  uint4 r[KV], a[KV], q[KV];
#pragma unroll
  for (int j = 0; j < KV; ++j) {
    r[j] = make_uint4(0, 0, 0, 0); a[j] = r[j]; q[j] = r[j];
    const int pix = p0 + pl + j * g.RL;
    if (on && pix < p1) {
      const int y = pix / g.W, xx = pix % g.W;
      r[j] = ldv<T>(x, b, y, xx, c);
      if (gr.has1) a[j] = ldv<T>(gr.g1, b, y, xx, c);
      if (gr.has2) q[j] = ldv<T>(gr.g2, b, y, xx, c);
    }
  }
  float mu[N], rs[N], ga[N], be[N], S[2 * N];
#pragma unroll
  for (int e = 0; e < N; ++e) { mu[e] = 0.f; rs[e] = 0.f; ga[e] = 1.f; be[e] = 0.f; }
  if (on) {
    ldc<N>(mean + (long long)b * g.C + c, mu);
    ldc<N>(rstd + (long long)b * g.C + c, rs);
    affine_of<N>(gamma, beta, c, ga, be);
  }
#pragma unroll
  for (int e = 0; e < 2 * N; ++e) S[e] = 0.f;
  if (MODE != 2) {
#pragma unroll
    for (int j = 0; j < KV; ++j)
      if (on && p0 + pl + j * g.RL < p1) {
        float dn[N], xh[N];
        dn_xhat<T, N>(gr, r[j], a[j], q[j], mu, rs, ga, be, dn, xh);
#pragma unroll
        for (int e = 0; e < N; ++e) { S[e] += dn[e]; S[N + e] = fmaf(dn[e], xh[e], S[N + e]); }
      }
    lane_tree<2 * N>(S, red, g, pl);
    if (MODE == 1) {
      if (on && pl == 0) {
#pragma unroll
        for (int e = 0; e < N; ++e)
          *reinterpret_cast<float2*>(part + (((long long)b * g.nchunks + ch) * g.C + c + e) * 2) = make_float2(S[e], S[N + e]);
      }
      return;
    }
  } else {
    if (on && pl == 0) {
      for (int k = 0; k < g.nchunks; ++k) {  // chunk order
        float pv[2 * N];
        ldc<2 * N>(part + (((long long)b * g.nchunks + k) * g.C + c) * 2, pv);
#pragma unroll
        for (int e = 0; e < N; ++e) { S[e] += pv[2 * e]; S[N + e] += pv[2 * e + 1]; }
      }
#pragma unroll
      for (int e = 0; e < 2 * N; ++e) red[cgl * 2 * N + e] = S[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 2 * N; ++e) S[e] = red[cgl * 2 * N + e];
  }
  if (!on) return;
  if (sums && pl == 0 && ch == 0) {
#pragma unroll
    for (int e = 0; e < N; ++e)
      *reinterpret_cast<float2*>(sums + ((long long)b * g.C + c + e) * 2) = make_float2(S[e], S[N + e]);
  }
  float k[N];
#pragma unroll
  for (int e = 0; e < N; ++e) { k[e] = ga[e] * rs[e]; S[e] = S[e] / (float)g.P; S[N + e] = S[N + e] / (float)g.P; }
#pragma unroll
  for (int j = 0; j < KV; ++j) {
    const int pix = p0 + pl + j * g.RL;
    if (pix < p1) {
      float dn[N], xh[N], d[N];
      dn_xhat<T, N>(gr, r[j], a[j], q[j], mu, rs, ga, be, dn, xh);
#pragma unroll
      for (int e = 0; e < N; ++e) d[e] = k[e] * (dn[e] - S[e] - xh[e] * S[N + e]);
      stv<T>(dx, b, pix / g.W, pix % g.W, c, Vec16<T>::pack(d));
    }
  }
}

// dbeta[c] = sum_b sums[b][c][0], dgamma[c] = sum_b sums[b][c][1], in sample order
__global__ void __launch_bounds__(256) in_param_grad_kernel(const float* sums, int B, int C, float* dgamma, float* dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s1 = 0.f, s2 = 0.f;
  for (int b = 0; b < B; ++b) {
    const float2 v = *reinterpret_cast<const float2*>(sums + ((long long)b * C + c) * 2);
    s1 += v.x;
    s2 += v.y;
  }
  dbeta[c] = s1;
  dgamma[c] = s2;
}

// ---------------------------------------------------------------- host
struct Plan {
  int regime;  // 0 tiny, 1 resident, 2 streamed
  Geo g;
  int nslab, m;
  long long part_bytes, sums_bytes;
};

static int lg2_ceil(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

static int make_plan(const char* who, int dtype, int B, int H, int W, int C, Plan* p) {
  STC_REQUIRE(dtype == STC_F32 || dtype == STC_BF16, "%s: unknown dtype %d", who, dtype);
  const int N = dtype == STC_F32 ? 4 : 8;
  STC_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "%s: bad extent B=%d H=%d W=%d", who, B, H, W);
  STC_REQUIRE(C >= N && C % N == 0, "%s: C=%d must be a multiple of %d (16-byte channel vectors)", who, C, N);
  STC_REQUIRE((long long)H * W < (1ll << 30), "%s: plane %dx%d too large", who, H, W);
  STC_REQUIRE((long long)H * W > 1, "%s: Expected more than 1 spatial element when training, got input size "
              "torch.Size([%d, %d, %d, %d])", who, B, C, H, W);
  Geo& g = p->g;
  g.W = W; g.P = H * W; g.C = C; g.CG = C / N;
  p->sums_bytes = (long long)B * C * 2 * sizeof(float);
  if (g.P <= TINY_MAX) {
    p->regime = 0;
    g.SV = 1; g.RL = 1; g.rl2 = 1; g.shfl = 0; g.pc = g.P; g.nchunks = 1;
    p->nslab = g.CG;
    p->m = g.P;
    p->part_bytes = 0;
    return 0;
  }
  g.SV = std::min(g.CG, SV_MAX);
  g.RL = NT / g.SV;
  g.rl2 = 1 << lg2_ceil(g.RL);
  g.shfl = 64 % g.SV == 0 ? 1 : 0;
  const int cap = g.RL * KV;
  g.nchunks = (g.P + cap - 1) / cap;
  g.pc = (g.P + g.nchunks - 1) / g.nchunks;
  g.nchunks = (g.P + g.pc - 1) / g.pc;
  p->nslab = (g.CG + g.SV - 1) / g.SV;
  STC_REQUIRE(p->nslab <= 65535, "%s: C=%d too wide", who, C);
  p->regime = g.nchunks == 1 ? 1 : 2;
  // a thread's own pixels in order, the tree over the pixel lanes, then the chunks in order
  // (with the wave butterfly: its levels, then the NT / 64 wave totals in order)
  const int lanes = g.shfl ? lg2_ceil(64 / g.SV) + NT / 64 : lg2_ceil(g.RL);
  p->m = (g.pc + g.RL - 1) / g.RL + lanes + (g.nchunks > 1 ? g.nchunks : 0);
  p->part_bytes = g.nchunks > 1 ? (long long)B * g.nchunks * C * 2 * sizeof(float) : 0;
  return 0;
}

static bool view_ok(int N, const stc_view& v) {
  return v.p && ((uintptr_t)v.p % 16) == 0 && v.cs == 1 && v.co % N == 0 && v.ps % N == 0 && v.rs % N == 0 &&
         v.bs % N == 0;
}
static bool same_extent(const stc_view& a, const stc_view& b) { return a.H == b.H && a.W == b.W; }

}  // namespace inorm
}  // namespace stc

using namespace stc;
using namespace stc::inorm;

extern "C" int stc_in_plan(int dtype, int B, int H, int W, int C, int32_t* out) {
  Plan p;
  if (int rc = make_plan("stc_in_plan", dtype, B, H, W, C, &p)) return rc;
  STC_REQUIRE(out, "stc_in_plan: out required");
  out[0] = p.regime;
  out[1] = p.g.SV * (dtype == STC_F32 ? 4 : 8);
  out[2] = p.g.nchunks;
  out[3] = p.m;
  return 0;
}

extern "C" int64_t stc_in_workspace(int dtype, int B, int H, int W, int C) {
  Plan p;
  if (make_plan("stc_in_workspace", dtype, B, H, W, C, &p)) return -1;
  return p.part_bytes + p.sums_bytes;
}

extern "C" int stc_in_fwd(int dtype, int B, stc_view x, int C, const float* gamma, const float* beta, float eps,
                          float* mean, float* rstd, stc_view apply_x, stc_view y1, float slope1, stc_view y2,
                          float slope2, void* ws, int64_t ws_bytes, void* stream) {
  Plan p;
  if (int rc = make_plan("stc_in_fwd", dtype, B, x.H, x.W, C, &p)) return rc;
  const int N = dtype == STC_F32 ? 4 : 8;
  STC_REQUIRE((gamma == nullptr) == (beta == nullptr), "stc_in_fwd: gamma/beta must come together");
  STC_REQUIRE(mean && rstd, "stc_in_fwd: mean/rstd outputs required");
  STC_REQUIRE(view_ok(N, x) && view_ok(N, y1) && (!y2.p || view_ok(N, y2)),
              "stc_in_fwd: views not 16-byte vectorisable NHWC");
  STC_REQUIRE(apply_x.p == x.p && apply_x.bs == x.bs && apply_x.rs == x.rs && apply_x.ps == x.ps &&
                  apply_x.co == x.co && apply_x.cs == x.cs && apply_x.H >= 1 && apply_x.W >= 1 &&
                  apply_x.H <= x.H && apply_x.W <= x.W,
              "stc_in_fwd: apply_x must be x or its top-left crop");
  STC_REQUIRE(same_extent(y1, apply_x) && (!y2.p || same_extent(y2, apply_x)),
              "stc_in_fwd: outputs must have apply_x's extent");
  STC_REQUIRE(p.part_bytes == 0 || (ws && ws_bytes >= p.part_bytes),
              "stc_in_fwd: workspace of %lld bytes required (stc_in_workspace), got %lld", p.part_bytes,
              (long long)ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  const View v = mkview(x);
  Outs o;
  o.y1 = mkview(y1); o.y2 = y2.p ? mkview(y2) : mkview(y1);
  o.s1 = slope1; o.s2 = slope2; o.has2 = y2.p ? 1 : 0; o.Ha = apply_x.H; o.Wa = apply_x.W;
  float* part = (float*)ws;
  const Geo& g = p.g;
  if (p.regime == 0) {
    const int blocks = cdiv((long long)B * g.CG, TINY_NT);
    STC_DT(dtype, hipLaunchKernelGGL(in_fwd_tiny_kernel<T_>, dim3(blocks), dim3(TINY_NT), 0, st, v, g, B, gamma, beta, eps, mean, rstd, o));
    STC_CHECK_LAUNCH();
    return 0;
  }
  const dim3 grid(g.nchunks, p.nslab, B);
#define STC_INF(M_) STC_DT(dtype, hipLaunchKernelGGL((in_fwd_kernel<T_, M_>), grid, dim3(NT), 0, st, v, g, gamma, beta, eps, mean, rstd, o, part))
  if (p.regime == 1) {
    STC_INF(0);
    STC_CHECK_LAUNCH();
    return 0;
  }
  STC_INF(1);
  STC_CHECK_LAUNCH();
  STC_INF(2);
#undef STC_INF
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_in_bwd(int dtype, int B, stc_view x, int C, const float* gamma, const float* beta,
                          const float* mean, const float* rstd, stc_view g1, float slope1, stc_view g2, float slope2,
                          stc_view dx, float* dgamma, float* dbeta, void* ws, int64_t ws_bytes, void* stream) {
  Plan p;
  if (int rc = make_plan("stc_in_bwd", dtype, B, x.H, x.W, C, &p)) return rc;
  const int N = dtype == STC_F32 ? 4 : 8;
  STC_REQUIRE((gamma == nullptr) == (beta == nullptr), "stc_in_bwd: gamma/beta must come together");
  STC_REQUIRE(mean && rstd, "stc_in_bwd: mean/rstd of the forward required");
  STC_REQUIRE(!gamma || (dgamma && dbeta), "stc_in_bwd: dgamma/dbeta required with an affine norm");
  STC_REQUIRE(view_ok(N, x) && view_ok(N, dx) && (!g1.p || view_ok(N, g1)) && (!g2.p || view_ok(N, g2)),
              "stc_in_bwd: views not 16-byte vectorisable NHWC");
  STC_REQUIRE(same_extent(dx, x) && (!g1.p || same_extent(g1, x)) && (!g2.p || same_extent(g2, x)),
              "stc_in_bwd: dx, g1 and g2 must cover x's extent");
  const long long need = p.part_bytes + (gamma ? p.sums_bytes : 0);
  STC_REQUIRE(need == 0 || (ws && ws_bytes >= need),
              "stc_in_bwd: workspace of %lld bytes required (stc_in_workspace), got %lld", need, (long long)ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  const View v = mkview(x), o = mkview(dx);
  Grads gr;
  gr.has1 = g1.p ? 1 : 0; gr.has2 = g2.p ? 1 : 0;
  gr.g1 = g1.p ? mkview(g1) : v; gr.g2 = g2.p ? mkview(g2) : v;
  gr.s1 = slope1; gr.s2 = slope2;
  float* part = (float*)ws;
  float* sums = gamma ? (float*)((char*)ws + p.part_bytes) : nullptr;
  const Geo& g = p.g;
  if (p.regime == 0) {
    const int blocks = cdiv((long long)B * g.CG, TINY_NT);
    STC_DT(dtype, hipLaunchKernelGGL(in_bwd_tiny_kernel<T_>, dim3(blocks), dim3(TINY_NT), 0, st, v, g, B, gamma, beta, mean, rstd, gr, o, sums));
    STC_CHECK_LAUNCH();
  } else {
    const dim3 grid(g.nchunks, p.nslab, B);
#define STC_INB(M_) STC_DT(dtype, hipLaunchKernelGGL((in_bwd_kernel<T_, M_>), grid, dim3(NT), 0, st, v, g, gamma, beta, mean, rstd, gr, o, part, sums))
    if (p.regime == 1) {
      STC_INB(0);
    } else {
      STC_INB(1);
      STC_CHECK_LAUNCH();
      STC_INB(2);
    }
#undef STC_INB
    STC_CHECK_LAUNCH();
  }
  if (gamma) {
    hipLaunchKernelGGL(in_param_grad_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, (const float*)sums, B, C, dgamma, dbeta);
    STC_CHECK_LAUNCH();
  }
  return 0;
}
