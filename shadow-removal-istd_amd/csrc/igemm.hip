// Implicit-GEMM 4x4 convolution family on gfx950 MFMA.
//
// One kernel template serves every forward product on the ST-CGAN path and
// both input gradients:
//   Conv2d k4 s2/s1 p1           : M = B*Ho*Wo, N = Cout, K = 16*Cin
//   ConvTranspose2d k4 s2 p1     : 4 sub-pixel phases, each M = B*Hi*Wi, N = Cout, K = 4*Cin
//   Conv-s2 dgrad == ConvT fwd geometry, ConvT dgrad == Conv-s2 geometry, Conv-s1 dgrad (flipped taps)
// A (activations, NHWC) is gathered on the fly: row m -> (b, y, x), k -> (tap, ci);
// tap offsets are affine in the tap index, so one parameter set describes every case.
// A per-channel affine + leaky prologue applies BatchNorm-apply and LeakyReLU/ReLU of
// the *producer* while loading (zero padding stays zero), so normalised activations
// are never materialised in HBM.
//
// Tile: BM x BN x (128 bytes of K) per stage, 256 threads = 4 waves, each wave a
// (BM/WM) x (BN/WN) sub-tile of 32x32 MFMA blocks.  LDS rows are 128 B of K plus
// 16 B of pad (144 B stride): the 16-lane groups of ds_read_b128 then hit 16
// distinct 16-byte bank slots (conflict-free).  fp32 uses v_mfma_f32_32x32x2_f32
// (4 MFMAs per 16-byte fragment, exact fp32 fmaf chains), bf16 uses
// v_mfma_f32_32x32x16_bf16 (1 MFMA per fragment); both read the same LDS image.
// Register-staged double buffer: the global loads of K-step s+1 are in flight
// while step s runs on MFMA; one barrier per step.
#include "common.hpp"
#include "conv_route.hpp"

namespace stc {

struct ConvParams {
  const char* a;
  long long a_bs, a_rs;
  int a_ps, a_co;
  int IH, IW;
  int cin, lg_tw, in_stride;
  int offy[4], offx[4];
  int stepy, stepx;
  const float* sc;
  const float* sh;
  int pro_act;
  float slope;
  int GH, GW, M, N, K;
  int ksplit, kchunk;
  const char* b;
  long long b_phase_stride;
  char* c;
  long long c_bs, c_rs;
  int c_ps, c_co, c_cs;
  int os;
  int oy0[4], ox0[4];
  const float* bias;
  int tanh_, out_f32;
  float* ws;
  int nphase;
  int mtiles, ntiles;
};

constexpr int LDS_ROW = 144;  // 128 B of K + 16 B pad

template <typename T>
__device__ __forceinline__ uint4 prologue16(uint4 v, const float* sc, const float* sh, int ci,
                                            int act_on, float slope) {
  constexpr int VEC = 16 / sizeof(T);
  float f[VEC];
  if constexpr (sizeof(T) == 4) {
    f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y);
    f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
  } else {
    unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f[2 * q] = __uint_as_float(w[q] << 16);
      f[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u);
    }
  }
  if (sc) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) f[e] = fmaf(f[e], sc[ci + e], sh[ci + e]);
  }
  if (act_on) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) f[e] = f[e] > 0.f ? f[e] : f[e] * slope;
  }
  uint4 r;
  if constexpr (sizeof(T) == 4) {
    r.x = __float_as_uint(f[0]); r.y = __float_as_uint(f[1]);
    r.z = __float_as_uint(f[2]); r.w = __float_as_uint(f[3]);
  } else {
    unsigned w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      w[q] = (unsigned)f2bf(f[2 * q]) | ((unsigned)f2bf(f[2 * q + 1]) << 16);
    r.x = w[0]; r.y = w[1]; r.z = w[2]; r.w = w[3];
  }
  return r;
}

// Reflect padding (STC_PAD_REFLECT): the one-wide halo of a Conv2d k4 p1 reads the plane
// mirrored about its border pixel, R(-1) = 1 and R(H) = H - 2 -- the only two out-of-range indices the taps reach.
// Any other index is returned as it came (rows past M stay out of bounds).
__device__ __forceinline__ int reflect1(int j, int H) { return j == -1 ? 1 : (j == H ? H - 2 : j); }

template <typename T, int BM, int BN, int WM, int WN, bool PRO>
__global__ void __launch_bounds__(256, 2)
igemm_kernel(const ConvParams p) {
#define STC_HALO_REMAP(iy, ix, IH, IW)
#include "igemm_tile.inc"
#undef STC_HALO_REMAP
}

// the same tile with the reflected halo (the engine materialises activations: no prologue form)
template <typename T, int BM, int BN, int WM, int WN>
__global__ void __launch_bounds__(256, 2)
igemm_reflect_kernel(const ConvParams p) {
  constexpr bool PRO = false;
#define STC_HALO_REMAP(iy, ix, IH, IW) iy = reflect1(iy, IH); ix = reflect1(ix, IW);
#include "igemm_tile.inc"
#undef STC_HALO_REMAP
}


// Split-K / raw-slab reduction with the epilogue: out[m, n] = epi(sum_s ws[ph][s][m][n])
template <typename T>
__global__ void splitk_reduce_kernel(const ConvParams p) {
  const long long total = (long long)p.nphase * p.M * p.N;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(idx % p.N);
    const long long pm = idx / p.N;
    const int m = (int)(pm % p.M);
    const int ph = (int)(pm / p.M);
    const float* src = p.ws + ((long long)ph * p.ksplit * p.M + m) * p.N + n;
    float v = 0.f;
    for (int s = 0; s < p.ksplit; ++s) v += src[(long long)s * p.M * p.N];
    if (p.bias) v += p.bias[n];
    v = head_act(v, p.tanh_);
    const int GHW = p.GH * p.GW;
    const int b = m / GHW, rem = m - b * GHW;
    const int y = rem / p.GW, x = rem - y * p.GW;
    const int oy = y * p.os + p.oy0[ph], ox = x * p.os + p.ox0[ph];
    const long long off = (long long)b * p.c_bs + (long long)oy * p.c_rs + (long long)ox * p.c_ps +
                          (long long)(p.c_co + n) * p.c_cs;
    if (p.out_f32) reinterpret_cast<float*>(p.c)[off] = v;
    else st1<T>(reinterpret_cast<T*>(p.c) + off, v);
  }
}

// Narrow-N layers (N <= 8: the 1/3-channel generator output, the 1-channel PatchGAN
// logits, first-layer input gradients).  An MFMA tile would waste >= 3/4 of its
// columns, and these layers are HBM-bound (K*4 B read per output pixel for <= 8
// outputs), so one wave computes one output pixel: its 64 lanes stride over the K
// chunks with coalesced 16-byte loads (1 KiB per wave instruction), the weights sit
// in LDS, and a wave shuffle reduces the N partial dots.
template <typename T>
__global__ void __launch_bounds__(256) smalln_kernel(const ConvParams p) {
#define STC_HALO_REMAP(iy, ix, IH, IW)
#include "smalln.inc"
#undef STC_HALO_REMAP
}

template <typename T>
__global__ void __launch_bounds__(256) smalln_reflect_kernel(const ConvParams p) {
#define STC_HALO_REMAP(iy, ix, IH, IW) iy = reflect1(iy, IH); ix = reflect1(ix, IW);
#include "smalln.inc"
#undef STC_HALO_REMAP
}


// Spatially tiled narrow-N kernel (the fast path for N <= 8).  One thread owns one
// GEMM-grid point (all 4 sub-pixel phases for the ConvT geometry); the block stages
// the input halo region for one 128-byte channel chunk in LDS (pixel stride 144 B:
// 16 lanes at consecutive pixels hit 16 distinct bank slots), so each input element
// is read from L2/HBM once per tile instead of once per output.  Weights are indexed
// only by loop counters (wave-uniform -> scalar / broadcast loads).
//   GEOM 0: ConvT-s2 phased geometry (taps in {0,1}^2 per phase, 3x3 neighbourhood),
//           TY x TX = 16 x 16 grid points, 256 threads.
//   GEOM 1: Conv k4 s1 (16 taps, 4x4 neighbourhood), 8 x 8 points, 64 threads.
template <typename T, int GEOM, int NMAX>
__global__ void narrow_tiled_kernel(const ConvParams p, int tiles_x, int tiles_per_img) {
  constexpr int TY = GEOM == 0 ? 16 : 8, TX = GEOM == 0 ? 16 : 8;
  constexpr int NT = TY * TX;
  constexpr int HALO = GEOM == 0 ? 2 : 3;  // region = (TY+HALO) x (TX+HALO), origin (-1,-1)
  constexpr int RY = TY + HALO, RX = TX + HALO;
  constexpr int VEC = 16 / sizeof(T);
  constexpr int CC = 128 / sizeof(T);  // channels per chunk
  constexpr int PSTR = 144;            // LDS bytes per staged pixel
  constexpr int NPH = GEOM == 0 ? 4 : 1;
  __shared__ __attribute__((aligned(16))) char tile[RY * RX * PSTR];

  const int tid = threadIdx.x;
  const int img = blockIdx.x / tiles_per_img, tix = blockIdx.x % tiles_per_img;
  const int y0 = (tix / tiles_x) * TY, x0 = (tix % tiles_x) * TX;
  const int ty = tid / TX, tx = tid % TX;
  const int gy = y0 + ty, gx = x0 + tx;
  const T* A = reinterpret_cast<const T*>(p.a) + (long long)img * p.a_bs + p.a_co;
  const T* Wt = reinterpret_cast<const T*>(p.b);
  const int taps = GEOM == 0 ? 4 : 16;

  float acc[NPH][NMAX];
#pragma unroll
  for (int q = 0; q < NPH; ++q)
#pragma unroll
    for (int n = 0; n < NMAX; ++n) acc[q][n] = 0.f;

  for (int c0 = 0; c0 < p.cin; c0 += CC) {
    // ---- stage the halo region (in-bounds pixels get the producer prologue)
    for (int i = tid; i < RY * RX * 8; i += NT) {
      const int pix = i >> 3, part = i & 7;
      const int ry = pix / RX, rx = pix - ry * RX;
      const int iy = y0 - 1 + ry, ix = x0 - 1 + rx;
      uint4 v = make_uint4(0, 0, 0, 0);
      if ((unsigned)iy < (unsigned)p.IH && (unsigned)ix < (unsigned)p.IW) {
        const int ci = c0 + part * VEC;
        v = *reinterpret_cast<const uint4*>(A + (long long)iy * p.a_rs + (long long)ix * p.a_ps + ci);
        if (p.sc || p.pro_act) v = prologue16<T>(v, p.sc, p.sh, ci, p.pro_act, p.slope);
      }
      *reinterpret_cast<uint4*>(tile + pix * PSTR + part * 16) = v;
    }
    __syncthreads();
    // ---- accumulate
#pragma unroll
    for (int part = 0; part < 8; ++part) {
      const int cbase = c0 + part * VEC;
      if constexpr (GEOM == 0) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const uint4 v = *reinterpret_cast<const uint4*>(tile + ((ty + 1 + dy) * RX + (tx + 1 + dx)) * PSTR + part * 16);
            float f[VEC];
            if constexpr (sizeof(T) == 4) {
              f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
            } else {
              const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
              for (int q = 0; q < 4; ++q) { f[2 * q] = __uint_as_float(w[q] << 16); f[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u); }
            }
#pragma unroll
            for (int ph = 0; ph < 2; ++ph)
#pragma unroll
              for (int pw = 0; pw < 2; ++pw) {
                const int th = ph - dy, tw = pw - dx;  // out(2y+ph) += in(y + ph - th) * w[tap th]
                if (th < 0 || th > 1 || tw < 0 || tw > 1) continue;
                const int phase = ph * 2 + pw, tap = th * 2 + tw;
#pragma unroll
                for (int n = 0; n < NMAX; ++n) {
                  if (n >= p.N) break;
                  const T* wr = Wt + p.b_phase_stride * phase + ((long long)n * taps + tap) * p.cin + cbase;
                  float s = acc[phase][n];
#pragma unroll
                  for (int e = 0; e < VEC; ++e) s = fmaf(f[e], ld1<T>(wr + e), s);
                  acc[phase][n] = s;
                }
              }
          }
      } else {
#pragma unroll
        for (int kh = 0; kh < 4; ++kh)
#pragma unroll
          for (int kw = 0; kw < 4; ++kw) {
            const uint4 v = *reinterpret_cast<const uint4*>(tile + ((ty + kh) * RX + (tx + kw)) * PSTR + part * 16);
            float f[VEC];
            if constexpr (sizeof(T) == 4) {
              f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
            } else {
              const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
              for (int q = 0; q < 4; ++q) { f[2 * q] = __uint_as_float(w[q] << 16); f[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u); }
            }
            const int tap = kh * 4 + kw;
#pragma unroll
            for (int n = 0; n < NMAX; ++n) {
              if (n >= p.N) break;
              const T* wr = Wt + ((long long)n * taps + tap) * p.cin + cbase;
              float s = acc[0][n];
#pragma unroll
              for (int e = 0; e < VEC; ++e) s = fmaf(f[e], ld1<T>(wr + e), s);
              acc[0][n] = s;
            }
          }
      }
    }
    __syncthreads();
  }
  if (gy >= p.GH || gx >= p.GW) return;
#pragma unroll
  for (int q = 0; q < NPH; ++q) {
    const int oy = gy * p.os + p.oy0[q], ox = gx * p.os + p.ox0[q];
    const long long base = (long long)img * p.c_bs + (long long)oy * p.c_rs + (long long)ox * p.c_ps;
#pragma unroll
    for (int n = 0; n < NMAX; ++n) {
      if (n >= p.N) break;
      float v = acc[q][n];
      if (p.bias) v += p.bias[n];
      v = head_act(v, p.tanh_);
      const long long off = base + (long long)(p.c_co + n) * p.c_cs;
      if (p.out_f32) reinterpret_cast<float*>(p.c)[off] = v;
      else st1<T>(reinterpret_cast<T*>(p.c) + off, v);
    }
  }
}

// narrow_tiled_kernel: ConvT s2 / conv s1, whole 128-byte channel chunks
bool narrow_tiled_eligible(int dtype, int kind, int Cin) {
  return (kind == STC_CONVT_S2 || kind == STC_CONV_S1) && Cin % (dtype == STC_F32 ? 32 : 64) == 0;
}

template <typename T>
static void launch_narrow_tiled(int kind, int B, ConvParams& p, hipStream_t st) {
  const int geom = kind == STC_CONVT_S2 ? 0 : 1;
  const int TY = geom == 0 ? 16 : 8, TX = geom == 0 ? 16 : 8;
  const int tiles_x = cdiv(p.GW, TX), tiles_y = cdiv(p.GH, TY);
  const int tpi = tiles_x * tiles_y;
  dim3 grid((unsigned)(B * tpi));
  const bool n4 = p.N <= 4;
  main_timer_begin(st);
  if (geom == 0) {
    if (n4) hipLaunchKernelGGL((narrow_tiled_kernel<T, 0, 4>), grid, dim3(256), 0, st, p, tiles_x, tpi);
    else hipLaunchKernelGGL((narrow_tiled_kernel<T, 0, 8>), grid, dim3(256), 0, st, p, tiles_x, tpi);
  } else {
    if (n4) hipLaunchKernelGGL((narrow_tiled_kernel<T, 1, 4>), grid, dim3(64), 0, st, p, tiles_x, tpi);
    else hipLaunchKernelGGL((narrow_tiled_kernel<T, 1, 8>), grid, dim3(64), 0, st, p, tiles_x, tpi);
  }
  main_timer_end(st);
}

// The fold of a reflect input gradient: frame[b][a + 1][c + 1][n] (fp32, FH x FW allocated) holds
// what pixel (a, c) of the extended grid -1 .. H, -1 .. W receives from the padding-free transposed conv; the input
// gradient at (y, x) is the sum over the frame pixels that reflect onto it -- its own, row -1 for y == 1, row H for
// y == H - 2 (both for H == 3; for H == 2 row 0 takes row H and row 1 row -1), columns alike: up to 3 x 3 fp32 values
// added in this fixed order, rounded once on store.  One thread = 4 channels of one pixel.
template <typename T>
__global__ void __launch_bounds__(256) reflect_fold_kernel(const float* __restrict__ frame, int FH, int FW, int N,
                                                           int B, int H, int W, char* c, long long c_bs,
                                                           long long c_rs, int c_ps, int c_co, int c_cs, int out_f32) {
  const int nq = N >> 2;
  const long long total = (long long)B * H * W * nq;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(idx % nq);
    long long pix = idx / nq;
    const int x = (int)(pix % W);
    pix /= W;
    const int y = (int)(pix % H), b = (int)(pix / H);
    int ry[3], rx[3], ny = 0, nx = 0;
    ry[ny++] = y + 1;
    if (y == 1) ry[ny++] = 0;
    if (y == H - 2) ry[ny++] = H + 1;
    rx[nx++] = x + 1;
    if (x == 1) rx[nx++] = 0;
    if (x == W - 2) rx[nx++] = W + 1;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = 0; i < ny; ++i)
      for (int j = 0; j < nx; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(frame + (((long long)b * FH + ry[i]) * FW + rx[j]) * N + 4 * q);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
    const long long off = (long long)b * c_bs + (long long)y * c_rs + (long long)x * c_ps;
    const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long o = off + (long long)(c_co + 4 * q + e) * c_cs;
      if (out_f32) reinterpret_cast<float*>(c)[o] = sv[e];
      else st1<T>(reinterpret_cast<T*>(c) + o, sv[e]);
    }
  }
}

// ------------------------------------------------------------------------- host
static int launch_reflect_fold(int dtype, int B, const ConvRoute& r, int N, const stc_view& y, bool out_f32,
                               const float* frame, hipStream_t st) {
  const long long work = (long long)B * y.H * y.W * (N / 4);
  STC_DT(dtype, hipLaunchKernelGGL(reflect_fold_kernel<T_>, dim3(grid_for(work)), dim3(256), 0, st, frame, r.FH, r.FW,
                                   N, B, y.H, y.W, (char*)y.p, (long long)y.bs, (long long)y.rs, y.ps, y.co, y.cs,
                                   (out_f32 || dtype == STC_F32) ? 1 : 0));
  STC_CHECK_LAUNCH();
  return 0;
}

static int ilog2_exact(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return (1 << l) == v ? l : -1;
}

FpPlan fp_tile_plan(int dtype, int M, int N, int K, int nphase) {
  const int BK = dtype == STC_F32 ? 32 : 64;
  FpPlan pl{};
  if (N <= 32) { pl.BM = 128; pl.BN = 32; }
  else if (N <= 64) { pl.BM = 128; pl.BN = 64; }
  else { pl.BM = 128; pl.BN = 128; }
  if (M <= 64 && N >= 128) { pl.BM = 32; pl.BN = 128; }
  else if (M <= 512 && N >= 64) { pl.BM = 64; pl.BN = 64; }
  pl.mtiles = cdiv(M, pl.BM);
  pl.ntiles = cdiv(N, pl.BN);
  const long long tiles = (long long)pl.mtiles * pl.ntiles * nphase;
  const int ksteps = cdiv(K, BK);
  int ks = 1;
  // split K until the grid covers the chip (~2 waves of 256 CUs), keeping >= 4 K-steps per split
  while (tiles * ks < 512 && ks * 2 <= 64 && ksteps / (ks * 2) >= 4) ks *= 2;
  pl.ksplit = ks;
  pl.kchunk = cdiv(ksteps, ks) * BK;
  pl.ksplit = cdiv(K, pl.kchunk);
  return pl;
}

static size_t lds_bytes(int BM, int BN) { return 2 * (size_t)(BM + BN) * LDS_ROW + BM * 8; }

template <typename T>
static int launch_igemm(const FpPlan& pl, ConvParams& p, hipStream_t st, bool reflect = false) {
  dim3 grid(pl.mtiles * pl.ntiles, 1, p.nphase * pl.ksplit);
  const size_t lds = lds_bytes(pl.BM, pl.BN);
  const bool pro = p.sc != nullptr || p.pro_act != 0;
  main_timer_begin(st);
#define STC_L(BM_, BN_, WM_, WN_)                                                                  \
  if (pl.BM == BM_ && pl.BN == BN_) {                                                              \
    if (reflect) hipLaunchKernelGGL((igemm_reflect_kernel<T, BM_, BN_, WM_, WN_>), grid, dim3(256), lds, st, p); \
    else if (pro) hipLaunchKernelGGL((igemm_kernel<T, BM_, BN_, WM_, WN_, true>), grid, dim3(256), lds, st, p); \
    else hipLaunchKernelGGL((igemm_kernel<T, BM_, BN_, WM_, WN_, false>), grid, dim3(256), lds, st, p);    \
  } else
  STC_L(128, 128, 2, 2)
  STC_L(128, 64, 2, 2)
  STC_L(128, 32, 4, 1)
  STC_L(64, 64, 2, 2)
  STC_L(32, 128, 1, 4)
  { return fail(-1, "igemm: no kernel for tile %dx%d", pl.BM, pl.BN); }
#undef STC_L
  main_timer_end(st);
  STC_CHECK_LAUNCH();
  if (p.ws) {
    const long long total = (long long)p.nphase * p.M * p.N;
    const int blocks = (int)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(splitk_reduce_kernel<T>, dim3(blocks), dim3(256), 0, st, p);
    STC_CHECK_LAUNCH();
  }
  return 0;
}

bool use_smalln(int dtype, int N, int K) {
  const int esz = dtype == STC_F32 ? 4 : 2;
  return N <= 8 && (long long)N * K * esz <= 64 * 1024;
}

}  // namespace stc

using namespace stc;

// ---- asks.  Every entry point below states its call as a ConvAsk, takes the route from conv_route (conv_route.cpp,
// DESIGN.md section 4) and reads its answer there or launches the kernel it names.
static ConvAsk conv_ask(int dtype, int kind, int B, const stc_view& x, int Cin, int Cout, const stc_view& y) {
  ConvAsk a{};
  a.dtype = dtype; a.kind = kind; a.B = B; a.x = x; a.y = y; a.Cin = Cin; a.Cout = Cout;
  return a;
}

// The views the shape-only queries assume, written down once: dense NHWC of the kind's input and output extents for
// the GEMM grid Hg x Wg, channel offset 0, 16-byte aligned base, no second gradient -- and batch stride 0: a shape
// has no allocation, so the limits the kernels put on a view's size in memory (2 GiB of input, 2^31 output elements,
// both growing with B * bs) count as met.  The _ex forms and the launches answer for the real views.
static ConvAsk shape_ask(int dtype, int kind, int B, int Hg, int Wg, int Cin, int Cout) {
  const int d = kind == STC_CONV_S1 ? 1 : (kind == STC_CONV_S1_DGRAD ? -1 : 0);  // conv s1: 31 x 31 from 32 x 32
  const stc_view grid = dense_view(Hg, Wg, kind == STC_CONVT_S2 ? Cin : Cout);
  const stc_view other = kind == STC_CONVT_S2 ? dense_view(2 * Hg, 2 * Wg, Cout)
                                              : (d ? dense_view(Hg + d, Wg + d, Cin) : dense_view(2 * Hg, 2 * Wg, Cin));
  return kind == STC_CONVT_S2 ? conv_ask(dtype, kind, B, grid, Cin, Cout, other)
                              : conv_ask(dtype, kind, B, other, Cin, Cout, grid);
}

// (the prologue form runs the register-staged kernel where the plain call runs a bf16 one: enough for both)
extern "C" int64_t stc_conv_fwd_workspace(int dtype, int kind, int B, int Hg, int Wg, int Cin, int Cout) {
  ConvAsk a = shape_ask(dtype, kind, B, Hg, Wg, Cin, Cout);
  const int64_t ws_plain = conv_route(a).ws_bytes;
  a.prologue = true;
  return std::max(ws_plain, conv_route(a).ws_bytes);
}

// out[0..3] = {BM, BN, ksplit, narrow-N path}; Hg x Wg is the GEMM grid (output grid for
// the conv kinds, input grid for STC_CONVT_S2).
extern "C" int stc_conv_fwd_plan(int dtype, int kind, int B, int Hg, int Wg, int Cin, int Cout, int32_t* out) {
  STC_REQUIRE(kind >= 0 && kind <= 3 && out, "stc_conv_fwd_plan: bad arguments");
  const ConvRoute r = conv_route(shape_ask(dtype, kind, B, Hg, Wg, Cin, Cout));
  for (int i = 0; i < 4; ++i) out[i] = r.plan[i];
  return 0;
}

// Forward conv with fused BatchNorm output statistics and an optional forced plan (tuning /
// tests).  stats_part: [chunks][Cout][4] in stc_chan_stats format (merged by stc_bn_finalize).
// plan_out[5] = {BM, BN, ksplit, narrow, cfg}.
extern "C" int stc_conv_fwd_query(int dtype, int kind, int B, int Hg, int Wg, int Cin, int Cout, int out_f32,
                                  const int32_t* force_plan, int64_t* workspace_bytes, int32_t* stats_chunks,
                                  int32_t* plan_out) {
  STC_REQUIRE(kind >= 0 && kind <= 3, "stc_conv_fwd_query: bad kind %d", kind);
  ConvAsk a = shape_ask(dtype, kind, B, Hg, Wg, Cin, Cout);
  a.out_f32 = out_f32 != 0;
  a.stats = true;
  a.force = force_plan;
  const ConvRoute r = conv_route(a);
  if (workspace_bytes) *workspace_bytes = r.ws_bytes;
  if (stats_chunks) *stats_chunks = r.chunks;
  if (plan_out)
    for (int i = 0; i < 5; ++i) plan_out[i] = r.plan[i];
  return 0;
}

// ---- launches
static int conv_fwd_checks(const ConvAsk& a, const ConvOps& o) {
  STC_REQUIRE(a.dtype == STC_F32 || a.dtype == STC_BF16, "stc_conv_fwd: bad dtype %d", a.dtype);
  STC_REQUIRE(a.kind >= 0 && a.kind <= 3, "stc_conv_fwd: bad kind %d", a.kind);
  const int VEC = a.dtype == STC_F32 ? 4 : 8;
  STC_REQUIRE(a.Cin >= VEC && a.Cin % VEC == 0, "stc_conv_fwd: Cin=%d must be a multiple of %d", a.Cin, VEC);
  STC_REQUIRE(a.x.co % VEC == 0 && a.x.ps % VEC == 0 && a.x.cs == 1, "stc_conv_fwd: input view must be NHWC, 16-byte aligned channels");
  STC_REQUIRE((o.pro_scale == nullptr) == (o.pro_shift == nullptr), "stc_conv_fwd: scale/shift must come together");
  return 0;
}

// the kernel r names, for an ask that passed conv_fwd_checks
static int conv_launch(const ConvAsk& a, const ConvRoute& r, const ConvOps& o) {
  const int dtype = a.dtype, kind = a.kind, B = a.B, Cin = a.Cin, Cout = a.Cout;
  const stc_view& x = a.x;
  const stc_view& y = a.y;
  if (B * r.GH * r.GW == 0 || Cout == 0) return 0;
  switch (r.kernel) {
    case STEM: case STEM_S1D: case HALO: case BF16_TILE:
      return bf16_conv_fwd(a, r, o);
    case BF16_NARROW:
      return bf16_narrow_fwd(kind, B, x, Cin, o.w, Cout, y, o.bias, a.tanh, a.out_f32, o.ws, o.ws_bytes, o.st,
                             r.narrow_force);
    case CONV_NONE:
      return fail(-1, "conv: no kernel for this call");
    default:
      break;
  }
  const Geometry g = geometry(kind);
  const int K = (g.taps_lg_tw == 2 ? 16 : 4) * Cin;
  ConvParams p{};
  p.a = (const char*)x.p; p.a_bs = x.bs; p.a_rs = x.rs; p.a_ps = x.ps; p.a_co = x.co;
  p.IH = x.H; p.IW = x.W;
  p.cin = Cin; p.lg_tw = g.taps_lg_tw; p.in_stride = g.in_stride;
  for (int i = 0; i < 4; ++i) { p.offy[i] = g.offy[i]; p.offx[i] = g.offx[i]; }
  p.stepy = g.stepy; p.stepx = g.stepx;
  p.sc = o.pro_scale; p.sh = o.pro_shift; p.pro_act = o.pro_act; p.slope = o.pro_slope;
  p.GH = r.GH; p.GW = r.GW; p.M = B * r.GH * r.GW; p.N = Cout; p.K = K;
  p.b = (const char*)o.w;
  p.b_phase_stride = (long long)Cout * K;
  p.c = (char*)y.p; p.c_bs = y.bs; p.c_rs = y.rs; p.c_ps = y.ps; p.c_co = y.co; p.c_cs = y.cs;
  p.os = g.os;
  for (int i = 0; i < 4; ++i) { p.oy0[i] = g.nphase == 4 ? (i >> 1) : 0; p.ox0[i] = g.nphase == 4 ? (i & 1) : 0; }
  p.bias = o.bias; p.tanh_ = a.tanh; p.out_f32 = a.out_f32 || dtype == STC_F32;
  p.nphase = g.nphase;
  // Reflect padding.  The forward is the reflect instantiation of the kernel the route names.
  // The input gradient is the padding-free transposed conv over the extended grid -1 .. H (r.GH x r.GW per phase):
  // the same kernels as ever with the tap origin moved by one (frame index f = a + 1; for the stride-2 form frame
  // row 2y + 1 is phase 0 and row 2y phase 1, both reading dy rows y - t) and an fp32 frame at the head of the
  // workspace as the output, then reflect_fold_kernel into y.
  const bool reflect_fwd = a.pad == STC_PAD_REFLECT && (kind == STC_CONV_S2 || kind == STC_CONV_S1);
  const bool frame = a.pad == STC_PAD_REFLECT && !reflect_fwd;
  char* ws = (char*)o.ws;
  if (frame) {
    STC_REQUIRE(o.ws && o.ws_bytes >= r.ws_bytes, "stc_conv_pad_dgrad: workspace %lld < %lld bytes",
                (long long)o.ws_bytes, (long long)r.ws_bytes);
    for (int i = 0; i < 4; ++i) {
      p.offy[i] = 0; p.offx[i] = 0;
      p.oy0[i] = g.nphase == 4 ? 1 - (i >> 1) : 0;
      p.ox0[i] = g.nphase == 4 ? 1 - (i & 1) : 0;
    }
    p.c = ws; p.c_bs = (long long)r.FH * r.FW * Cout; p.c_rs = (long long)r.FW * Cout; p.c_ps = Cout; p.c_co = 0;
    p.c_cs = 1;
    p.bias = nullptr; p.tanh_ = 0; p.out_f32 = 1;
    ws += r.frame_bytes;
  }
  if (r.kernel == FP_TILE) {
    const FpPlan& pl = r.fp;
    p.ksplit = pl.ksplit; p.kchunk = pl.kchunk; p.mtiles = pl.mtiles; p.ntiles = pl.ntiles;
    if (pl.ksplit > 1) {
      STC_REQUIRE(o.ws && o.ws_bytes >= r.ws_bytes, "stc_conv_fwd: workspace %lld < %lld bytes",
                  (long long)o.ws_bytes, (long long)r.ws_bytes);
      p.ws = (float*)ws;
    }
    const int rc = dtype == STC_F32 ? launch_igemm<float>(pl, p, o.st, reflect_fwd)
                                    : launch_igemm<bf16>(pl, p, o.st, reflect_fwd);
    if (rc || !frame) return rc;
    return launch_reflect_fold(dtype, B, r, Cout, y, a.out_f32, (const float*)o.ws, o.st);
  }
  p.mtiles = 1; p.ntiles = 1; p.ksplit = 1; p.kchunk = K;
  STC_REQUIRE(K % (dtype == STC_F32 ? 4 : 8) == 0, "stc_conv_fwd: K=%d", K);
  if (r.kernel == NARROW_TILED) {
    STC_DT(dtype, launch_narrow_tiled<T_>(kind, B, p, o.st));
  } else {  // SMALLN
    dim3 grid((unsigned)std::min(cdiv(p.M, 4), 4096), g.nphase);
    const size_t lds = (size_t)Cout * K * (dtype == STC_F32 ? 4 : 2);
    main_timer_begin(o.st);
    if (reflect_fwd) {
      STC_DT(dtype, hipLaunchKernelGGL(smalln_reflect_kernel<T_>, grid, dim3(256), lds, o.st, p));
    } else {
      STC_DT(dtype, hipLaunchKernelGGL(smalln_kernel<T_>, grid, dim3(256), lds, o.st, p));
    }
    main_timer_end(o.st);
  }
  STC_CHECK_LAUNCH();
  if (frame) return launch_reflect_fold(dtype, B, r, Cout, y, a.out_f32, (const float*)o.ws, o.st);
  return 0;
}

// checks, route, launch; statistics the kernel does not compute itself come from stc_chan_stats over its output.
// stc_conv_fwd checks its arguments first; stc_conv_fwd_ex (kind checked) hands the bf16 family and the narrow tuning
// hook to launchers that check their own, and runs these checks for the other routes only
static int conv_fwd(const ConvAsk& a, ConvOps o, bool ex) {
  if (!ex)
    if (const int rc = conv_fwd_checks(a, o)) return rc;
  const ConvRoute r = conv_route(a);
  if (ex && !r.fused && !r.narrow_force)
    if (const int rc = conv_fwd_checks(a, o)) return rc;
  float* const stats_after = r.fused ? nullptr : o.stats;
  if (!r.fused) o.stats = nullptr;
  const int rc = conv_launch(a, r, o);
  if (rc != 0 || stats_after == nullptr) return rc;
  STC_REQUIRE(!a.out_f32 || a.dtype == STC_F32, "stc_conv_fwd_ex: stats of a non-activation output");
  return stc_chan_stats(a.dtype, a.B, a.y, a.Cout, stats_after, o.stats_chunks, o.st);
}

extern "C" int stc_conv_fwd_ex(int dtype, int kind, int B, stc_view x, int Cin, const void* w_packed, int Cout,
                               stc_view y, const float* bias, int epi_tanh, int out_f32, float* stats_part,
                               int stats_chunks, const int32_t* force_plan, void* workspace, int64_t workspace_bytes,
                               void* stream) {
  STC_REQUIRE(kind >= 0 && kind <= 3, "stc_conv_fwd_ex: bad kind %d", kind);
  STC_REQUIRE(head_code_ok(epi_tanh), "stc_conv_fwd_ex: epilogue code %d is none of STC_HEAD_* (0..3)", epi_tanh);
  ConvAsk a = conv_ask(dtype, kind, B, x, Cin, Cout, y);
  a.tanh = epi_tanh; a.out_f32 = out_f32 != 0; a.stats = stats_part != nullptr; a.force = force_plan;
  ConvOps o{};
  o.w = w_packed; o.bias = bias; o.stats = stats_part; o.stats_chunks = stats_chunks;
  o.ws = workspace; o.ws_bytes = workspace_bytes; o.st = (hipStream_t)stream;
  return conv_fwd(a, o, true);
}

// conv + BatchNorm (train mode) + activation as one call: stc_conv_fwd_ex with the batch statistics, stc_bn_finalize,
// stc_bn_apply -- the three launches of a BN layer's forward, enqueued by one host call (the train step makes ~50
// of them; each separate call costs host time the GPU then waits for).  fws = [stats partials nchunks*Cout*4 |
// mean | rstd | scale | shift] (Cout each); y1.p == NULL: no apply (the caller only needs the statistics).
extern "C" int stc_conv_bn_fwd(int dtype, int kind, int B, stc_view x, int Cin, const void* w_packed, int Cout,
                               stc_view y, float* fws, int nchunks, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                               float eps, stc_view apply_x, stc_view y1, float slope1, stc_view y2, float slope2,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  STC_REQUIRE(fws && nchunks > 0 && gamma && beta, "stc_conv_bn_fwd: statistics workspace and BN affine required");
  int rc = stc_conv_fwd_ex(dtype, kind, B, x, Cin, w_packed, Cout, y, nullptr, 0, 0, fws, nchunks, nullptr, workspace,
                           workspace_bytes, stream);
  if (rc) return rc;
  float* tab = fws + (int64_t)nchunks * Cout * 4;
  rc = stc_bn_finalize(fws, nchunks, Cout, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps,
                       tab, tab + Cout, tab + 2 * Cout, tab + 3 * Cout, stream);
  if (rc || !y1.p) return rc;
  return stc_bn_apply(dtype, B, apply_x, Cout, tab + 2 * Cout, tab + 3 * Cout, y1, slope1, y2, slope2, stream);
}

extern "C" int stc_conv_fwd(int dtype, int kind, int B, stc_view x, int Cin,
                            const float* pro_scale, const float* pro_shift, int pro_act, float pro_slope,
                            const void* w_packed, int Cout, stc_view y,
                            const float* bias, int epi_tanh, int out_f32,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  STC_REQUIRE(head_code_ok(epi_tanh), "stc_conv_fwd: epilogue code %d is none of STC_HEAD_* (0..3)", epi_tanh);
  ConvAsk a = conv_ask(dtype, kind, B, x, Cin, Cout, y);
  a.prologue = pro_scale != nullptr || pro_act != 0; a.tanh = epi_tanh; a.out_f32 = out_f32 != 0;
  ConvOps o{};
  o.w = w_packed; o.bias = bias;
  o.pro_scale = pro_scale; o.pro_shift = pro_shift; o.pro_act = pro_act; o.pro_slope = pro_slope;
  o.ws = workspace; o.ws_bytes = workspace_bytes; o.st = (hipStream_t)stream;
  return conv_fwd(a, o, false);
}

// ---- input-gradient conv + fused BN-backward reduction
static ConvAsk bwd_bn_ask(int dtype, int kind, int B, const stc_view& dy, int Cin, int Cout, const stc_view& out,
                          const stc_bnb_fuse* bnb) {
  ConvAsk a = conv_ask(dtype, kind, B, dy, Cin, Cout, out);
  a.bnb = bnb;
  return a;
}

// the part2 chunk count of stc_conv_bwd_bn for these exact views (the kernel route depends on the layout)
extern "C" int stc_conv_bwd_bn_chunks_ex(int dtype, int kind, int B, stc_view dy, int Cin, int Cout, stc_view out,
                                         const stc_bnb_fuse* bnb) {
  if (!bnb || kind < 0 || kind > 3) return fail(-1, "stc_conv_bwd_bn_chunks_ex: bad arguments"), 0;
  return conv_route(bwd_bn_ask(dtype, kind, B, dy, Cin, Cout, out, bnb)).chunks;
}

// (shape-only form: the views of shape_ask, the BN input dense over xH x xW -- stc_conv_bwd_bn_chunks_ex answers for
// the actual views)
extern "C" int stc_conv_bwd_bn_chunks(int dtype, int kind, int B, int Hg, int Wg, int Cin, int Cout, int xH, int xW) {
  stc_bnb_fuse f{};
  f.x = dense_view(xH, xW, Cout);
  f.C = Cout;
  ConvAsk a = shape_ask(dtype, kind, B, Hg, Wg, Cin, Cout);
  a.bnb = &f;
  return conv_route(a).chunks;
}

extern "C" int stc_conv_bwd_bn(int dtype, int kind, int B, stc_view dy, int Cin, const void* w_packed, int Cout,
                               stc_view out, const stc_bnb_fuse* bnb, float* part2, int nchunks, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  STC_REQUIRE(bnb && part2, "stc_conv_bwd_bn: bnb and part2 required");
  ConvAsk a = bwd_bn_ask(dtype, kind, B, dy, Cin, Cout, out, bnb);
  const ConvRoute r = conv_route(a);
  ConvOps o{};
  o.w = w_packed; o.ws = workspace; o.ws_bytes = workspace_bytes; o.st = (hipStream_t)stream;
  if (r.fused) {
    STC_REQUIRE(nchunks == r.chunks, "stc_conv_bwd_bn: %d chunks != %d (use stc_conv_bwd_bn_chunks_ex)", nchunks, r.chunks);
    o.part2 = part2; o.stats_chunks = r.chunks;
    return bf16_conv_fwd(a, r, o);
  }
  a.bnb = nullptr;  // the plain conv (r is its route), then the reduction over its output
  int rc = conv_fwd_checks(a, o);
  if (rc == 0) rc = conv_launch(a, r, o);
  if (rc) return rc;
  stc_view g1 = out;  // this conv's output, at the BN channels, over the BN extent
  g1.co += bnb->ch_off;
  g1.H = bnb->x.H;
  g1.W = bnb->x.W;
  STC_REQUIRE(nchunks == r.chunks, "stc_conv_bwd_bn: %d chunks != %d (use stc_conv_bwd_bn_chunks_ex)", nchunks, r.chunks);
  return stc_bn_bwd_reduce(dtype, B, bnb->x, bnb->C, bnb->scale, bnb->shift, bnb->mean, bnb->rstd, g1, bnb->slope_self,
                           bnb->g_other, bnb->slope_other, part2, r.chunks, stream);
}

// stc_conv_bwd_bn followed by its stc_bn_bwd_apply (the conv output at the BN channels over the BN extent as the
// first gradient): a BN layer's whole input-gradient step from one host call
extern "C" int stc_conv_bwd_bn_apply(int dtype, int kind, int B, stc_view dy, int Cin, const void* w_packed, int Cout,
                                     stc_view out, const stc_bnb_fuse* bnb, float* part2, int nchunks,
                                     const float* gamma, stc_view dx, float* dgamma, float* dbeta, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  int rc = stc_conv_bwd_bn(dtype, kind, B, dy, Cin, w_packed, Cout, out, bnb, part2, nchunks, workspace,
                           workspace_bytes, stream);
  if (rc) return rc;
  stc_view g1 = out;
  g1.co += bnb->ch_off;
  g1.H = bnb->x.H;
  g1.W = bnb->x.W;
  return stc_bn_bwd_apply(dtype, B, bnb->x, bnb->C, bnb->scale, bnb->shift, bnb->mean, bnb->rstd, gamma, g1,
                          bnb->slope_self, bnb->g_other, bnb->slope_other, part2, nchunks, dx, dgamma, dbeta, stream);
}

// ---- input-gradient conv + activation backward (layers without BatchNorm): the halo kernels' BN-backward epilogue
// with no table (f: the activation's input and the second gradient, filled here)
static ConvAsk bwd_act_ask(int dtype, int kind, int B, const stc_view& dy, int Cin, int Cout, const stc_view& out,
                           const stc_view& x, const stc_view& g_other, stc_bnb_fuse& f) {
  f.x = x;
  f.g_other = g_other;
  f.C = Cout;
  f.ch_off = 0;
  ConvAsk a = conv_ask(dtype, kind, B, dy, Cin, Cout, out);
  a.bnb = &f;
  a.bnb_act = true;
  return a;
}

extern "C" int stc_conv_bwd_act_ok(int dtype, int kind, int B, stc_view dy, int Cin, int Cout, stc_view out, stc_view x,
                                   stc_view g_other) {
  if (kind < 0 || kind > 3) return 0;
  stc_bnb_fuse f{};
  return conv_route(bwd_act_ask(dtype, kind, B, dy, Cin, Cout, out, x, g_other, f)).kernel == HALO ? 1 : 0;
}

extern "C" int stc_conv_bwd_act(int dtype, int kind, int B, stc_view dy, int Cin, const void* w_packed, int Cout,
                                stc_view out, stc_view x, float slope_self, stc_view g_other, float slope_other,
                                void* stream) {
  stc_bnb_fuse f{};
  f.slope_self = slope_self;
  f.slope_other = slope_other;
  const ConvAsk a = bwd_act_ask(dtype, kind, B, dy, Cin, Cout, out, x, g_other, f);
  ConvRoute r{};
  if (kind >= 0 && kind <= 3) r = conv_route(a);
  STC_REQUIRE(r.kernel == HALO,
              "stc_conv_bwd_act: no fused activation backward for this shape / view (check stc_conv_bwd_act_ok)");
  ConvOps o{};
  o.w = w_packed; o.st = (hipStream_t)stream;
  return bf16_conv_fwd(a, r, o);
}

// ---- conv + activation epilogue (layers without BatchNorm): the stem kernel, or the bf16 tile as one launch
static ConvAsk fwd_act_ask(int dtype, int kind, int B, const stc_view& x, int Cin, int Cout, const stc_view& y1,
                           const stc_view& y2) {
  ConvAsk a = conv_ask(dtype, kind, B, x, Cin, Cout, y1);
  a.act_n = y2.p ? 2 : 1;
  a.act2 = &y2;
  return a;
}
static bool fwd_act_ok(const ConvRoute& r) {
  return r.kernel == STEM || (r.kernel == BF16_TILE && r.bf.pl.ksplit == 1);
}

extern "C" int stc_conv_fwd_act_ok(int dtype, int kind, int B, stc_view x, int Cin, int Cout, stc_view y1, stc_view y2) {
  if (kind < 0 || kind > 3) return 0;
  return fwd_act_ok(conv_route(fwd_act_ask(dtype, kind, B, x, Cin, Cout, y1, y2))) ? 1 : 0;
}

extern "C" int stc_conv_fwd_act(int dtype, int kind, int B, stc_view x, int Cin, const void* w_packed, int Cout,
                                stc_view y1, float slope1, stc_view y2, float slope2, const float* bias,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  const ConvAsk a = fwd_act_ask(dtype, kind, B, x, Cin, Cout, y1, y2);
  ConvRoute r{};
  if (kind >= 0 && kind <= 3) r = conv_route(a);
  STC_REQUIRE(fwd_act_ok(r),
              "stc_conv_fwd_act: no activation epilogue for this shape (check stc_conv_fwd_act_ok)");
  ConvOps o{};
  o.w = w_packed; o.bias = bias; o.act_s1 = slope1; o.act_s2 = slope2;
  o.ws = workspace; o.ws_bytes = workspace_bytes; o.st = (hipStream_t)stream;
  return bf16_conv_fwd(a, r, o);
}


// ---- Conv2d k4 p1 with a padding mode (include/stcgan_hip.h).  STC_PAD_ZEROS: the entry points
// above, bit for bit.  STC_PAD_REFLECT: an ask with pad set -- conv_route sends it to the two gather kernels and fuses
// nothing.  Everything is judged here, before the first launch.
static int pad_checks(const char* who, int dtype, int kind, int pad_mode) {
  STC_REQUIRE(dtype == STC_F32 || dtype == STC_BF16, "%s: bad dtype %d", who, dtype);
  STC_REQUIRE(kind == STC_CONV_S2 || kind == STC_CONV_S1, "%s: kind %d is not a Conv2d kind (STC_CONV_S2, STC_CONV_S1)",
              who, kind);
  STC_REQUIRE(pad_mode == STC_PAD_ZEROS || pad_mode == STC_PAD_REFLECT,
              "%s: pad_mode %d is neither STC_PAD_ZEROS nor STC_PAD_REFLECT", who, pad_mode);
  return 0;
}
static int reflect_extent_check(const char* who, int H, int W) {
  STC_REQUIRE(H >= 2 && W >= 2,
              "%s: reflect padding needs an input extent >= 2 in both dimensions, got %d x %d (Padding size should be "
              "less than the corresponding input dimension)", who, H, W);
  return 0;
}
static int conv_out_extent(int h, int kind) { return kind == STC_CONV_S2 ? (h - 2) / 2 + 1 : h - 1; }
static int dgrad_kind(int kind) { return kind == STC_CONV_S2 ? STC_CONVT_S2 : STC_CONV_S1_DGRAD; }

extern "C" int stc_conv_pad_fwd_query(int dtype, int kind, int pad_mode, int B, int H, int W, int Cin, int Cout,
                                      int out_f32, const int32_t* force_plan, int64_t* workspace_bytes,
                                      int32_t* stats_chunks, int32_t* plan_out) {
  if (const int rc = pad_checks("stc_conv_pad_fwd_query", dtype, kind, pad_mode)) return rc;
  const int Ho = conv_out_extent(H, kind), Wo = conv_out_extent(W, kind);
  if (pad_mode == STC_PAD_ZEROS)
    return stc_conv_fwd_query(dtype, kind, B, Ho, Wo, Cin, Cout, out_f32, force_plan, workspace_bytes, stats_chunks,
                              plan_out);
  if (const int rc = reflect_extent_check("stc_conv_pad_fwd_query", H, W)) return rc;
  STC_REQUIRE(!force_plan, "stc_conv_pad_fwd_query: no plan can be forced under STC_PAD_REFLECT (force_plan must be NULL)");
  ConvAsk a = conv_ask(dtype, kind, B, dense_view(H, W, Cin), Cin, Cout, dense_view(Ho, Wo, Cout));
  a.out_f32 = out_f32 != 0;
  a.stats = true;
  a.pad = STC_PAD_REFLECT;
  const ConvRoute r = conv_route(a);
  if (workspace_bytes) *workspace_bytes = r.ws_bytes;
  if (stats_chunks) *stats_chunks = r.chunks;
  if (plan_out)
    for (int i = 0; i < 5; ++i) plan_out[i] = r.plan[i];
  return 0;
}

extern "C" int stc_conv_pad_fwd(int dtype, int kind, int pad_mode, int B, stc_view x, int Cin, const void* w_packed,
                                int Cout, stc_view y, const float* bias, int epi_tanh, int out_f32, float* stats_part,
                                int stats_chunks, const int32_t* force_plan, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  if (const int rc = pad_checks("stc_conv_pad_fwd", dtype, kind, pad_mode)) return rc;
  STC_REQUIRE(x.p && w_packed && y.p, "stc_conv_pad_fwd: null operand");
  if (pad_mode == STC_PAD_ZEROS)
    return stc_conv_fwd_ex(dtype, kind, B, x, Cin, w_packed, Cout, y, bias, epi_tanh, out_f32, stats_part,
                           stats_chunks, force_plan, workspace, workspace_bytes, stream);
  STC_REQUIRE(head_code_ok(epi_tanh), "stc_conv_pad_fwd: epilogue code %d is none of STC_HEAD_* (0..3)", epi_tanh);
  if (const int rc = reflect_extent_check("stc_conv_pad_fwd", x.H, x.W)) return rc;
  STC_REQUIRE(!force_plan, "stc_conv_pad_fwd: no plan can be forced under STC_PAD_REFLECT (force_plan must be NULL)");
  STC_REQUIRE(y.H == conv_out_extent(x.H, kind) && y.W == conv_out_extent(x.W, kind),
              "stc_conv_pad_fwd: y %d x %d is not the k4 s%d p1 output of x %d x %d", y.H, y.W,
              kind == STC_CONV_S2 ? 2 : 1, x.H, x.W);
  ConvAsk a = conv_ask(dtype, kind, B, x, Cin, Cout, y);
  a.tanh = epi_tanh; a.out_f32 = out_f32 != 0; a.stats = stats_part != nullptr; a.pad = STC_PAD_REFLECT;
  ConvOps o{};
  o.w = w_packed; o.bias = bias; o.ws = workspace; o.ws_bytes = workspace_bytes; o.st = (hipStream_t)stream;
  if (const int rc = conv_fwd_checks(a, o)) return rc;
  const ConvRoute r = conv_route(a);
  STC_REQUIRE(!stats_part || !a.out_f32 || dtype == STC_F32, "stc_conv_pad_fwd: stats of a non-activation output");
  STC_REQUIRE(r.ws_bytes == 0 || (workspace && workspace_bytes >= r.ws_bytes),
              "stc_conv_pad_fwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)r.ws_bytes);
  const int rc = conv_launch(a, r, o);
  if (rc != 0 || stats_part == nullptr) return rc;
  return stc_chan_stats(dtype, B, y, Cout, stats_part, stats_chunks, (hipStream_t)stream);
}

extern "C" int stc_conv_pad_dgrad_query(int dtype, int kind, int pad_mode, int B, int H, int W, int Cout, int Cin,
                                        int out_f32, int64_t* workspace_bytes, int32_t* plan_out) {
  if (const int rc = pad_checks("stc_conv_pad_dgrad_query", dtype, kind, pad_mode)) return rc;
  const int Ho = conv_out_extent(H, kind), Wo = conv_out_extent(W, kind);
  if (pad_mode == STC_PAD_ZEROS)  // (the grid of STC_CONVT_S2 is its input dy, of STC_CONV_S1_DGRAD its output dx)
    return stc_conv_fwd_query(dtype, dgrad_kind(kind), B, kind == STC_CONV_S2 ? Ho : H, kind == STC_CONV_S2 ? Wo : W,
                              Cout, Cin, out_f32, nullptr, workspace_bytes, nullptr, plan_out);
  if (const int rc = reflect_extent_check("stc_conv_pad_dgrad_query", H, W)) return rc;
  ConvAsk a = conv_ask(dtype, dgrad_kind(kind), B, dense_view(Ho, Wo, Cout), Cout, Cin, dense_view(H, W, Cin));
  a.out_f32 = out_f32 != 0;
  a.pad = STC_PAD_REFLECT;
  const ConvRoute r = conv_route(a);
  if (workspace_bytes) *workspace_bytes = r.ws_bytes;
  if (plan_out)
    for (int i = 0; i < 5; ++i) plan_out[i] = r.plan[i];
  return 0;
}

extern "C" int stc_conv_pad_dgrad(int dtype, int kind, int pad_mode, int B, stc_view dy, int Cout, const void* w_packed,
                                  int Cin, stc_view dx, int out_f32, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  if (const int rc = pad_checks("stc_conv_pad_dgrad", dtype, kind, pad_mode)) return rc;
  STC_REQUIRE(dy.p && w_packed && dx.p, "stc_conv_pad_dgrad: null operand");
  if (pad_mode == STC_PAD_ZEROS)
    return stc_conv_fwd_ex(dtype, dgrad_kind(kind), B, dy, Cout, w_packed, Cin, dx, nullptr, 0, out_f32, nullptr, 0,
                           nullptr, workspace, workspace_bytes, stream);
  if (const int rc = reflect_extent_check("stc_conv_pad_dgrad", dx.H, dx.W)) return rc;
  STC_REQUIRE(dy.H == conv_out_extent(dx.H, kind) && dy.W == conv_out_extent(dx.W, kind),
              "stc_conv_pad_dgrad: dy %d x %d is not the k4 s%d p1 output of dx %d x %d", dy.H, dy.W,
              kind == STC_CONV_S2 ? 2 : 1, dx.H, dx.W);
  STC_REQUIRE(Cin >= 4 && Cin % 4 == 0, "stc_conv_pad_dgrad: Cin=%d must be a multiple of 4", Cin);
  ConvAsk a = conv_ask(dtype, dgrad_kind(kind), B, dy, Cout, Cin, dx);
  a.out_f32 = out_f32 != 0;
  a.pad = STC_PAD_REFLECT;
  ConvOps o{};
  o.w = w_packed; o.ws = workspace; o.ws_bytes = workspace_bytes; o.st = (hipStream_t)stream;
  if (const int rc = conv_fwd_checks(a, o)) return rc;
  const ConvRoute r = conv_route(a);
  STC_REQUIRE(workspace && workspace_bytes >= r.ws_bytes, "stc_conv_pad_dgrad: workspace %lld < %lld bytes",
              (long long)workspace_bytes, (long long)r.ws_bytes);
  return conv_launch(a, r, o);
}
