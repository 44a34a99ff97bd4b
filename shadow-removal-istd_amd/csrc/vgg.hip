// The element-wise and reduction kernels of VisualLoss (src/loss.py:29-56 of the reference's src/ line) around the
// 3x3 convolutions of conv3_bf16.hip: the weight pack, MaxPool2d(2, 2) forward / backward, the ImageNet input
// normalisation and its backward, and the MSE between two bf16 feature tensors with its gradient.  NHWC bf16,
// 16-byte vectors; every sum in a fixed order (no atomics).
#include <algorithm>

#include "common.hpp"
#include "vec16.hpp"

namespace stc {

static inline int vgg_grid(long long n) { return (int)std::min<long long>((n + 255) / 256, 1 << 20); }

// ------------------------------------------------------------------ weight pack
struct Pack3Args {
  stc_conv3_pack_desc d[STC_CONV3_PACK_MAX];
};

// fwd[(n * 9 + t) * Ci_pad + c] = W[n][c][t];  dgrad[(m * 9 + t) * Co_pad + k] = W[k][m][8 - t] (taps flipped, ci / co
// swapped); padding entries zero.  RNE to bf16.
__global__ void pack3_kernel(const Pack3Args a) {
  const stc_conv3_pack_desc d = a.d[blockIdx.y];
  const long long tot = 9ll * d.Co_pad * d.Ci_pad;
  bf16* fwd = reinterpret_cast<bf16*>(d.fwd);
  bf16* dg = reinterpret_cast<bf16*>(d.dgrad);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * tot; i += (long long)gridDim.x * blockDim.x) {
    if (i < tot) {
      if (!fwd) continue;
      const int c = (int)(i % d.Ci_pad), t = (int)((i / d.Ci_pad) % 9), n = (int)(i / (9ll * d.Ci_pad));
      st1<bf16>(fwd + i, n < d.Co && c < d.Ci ? d.W[((long long)n * d.Ci + c) * 9 + t] : 0.f);
    } else {
      if (!dg) continue;
      const long long q = i - tot;
      const int k = (int)(q % d.Co_pad), t = (int)((q / d.Co_pad) % 9), m = (int)(q / (9ll * d.Co_pad));
      st1<bf16>(dg + q, k < d.Co && m < d.Ci ? d.W[((long long)k * d.Ci + m) * 9 + (8 - t)] : 0.f);
    }
  }
}

// ------------------------------------------------------------------ max-pool 2x2 s2
__device__ __forceinline__ const uint4* vec_at(const View& v, int b, int y, int x, int c) {
  return reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(v.p) + vidx(v, b, y, x, c));
}

// torch's rule (max_pool2d): scan (0,0), (0,1), (1,0), (1,1); an element replaces the maximum when it is greater or NaN
// -- the first maximal element wins a tie.  BWD: the gradient of each window goes to that position of gx, zeros to the
// other three (every element of gx is written: H and W are even).
template <bool BWD>
__global__ void pool2_kernel(int B, int OH, int OW, int C8, View x, View y, View g, View gx) {
  const long long total = (long long)B * OH * OW * C8;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C8) * 8;
    long long r = i / C8;
    const int ox = (int)(r % OW);
    r /= OW;
    const int oy = (int)(r % OH), b = (int)(r / OH);
    float v[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k) Vec16<bf16>::unpack(*vec_at(x, b, 2 * oy + (k >> 1), 2 * ox + (k & 1), c), v[k]);
    float m[8];
    int am[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      m[e] = v[0][e];
      am[e] = 0;
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (v[k][e] > m[e] || v[k][e] != v[k][e]) { m[e] = v[k][e]; am[e] = k; }
    }
    if constexpr (!BWD) {
      // (the values are bf16 already: the pack is exact)
      *const_cast<uint4*>(vec_at(y, b, oy, ox, c)) = make_uint4(pack_bf16x2(m[0], m[1]), pack_bf16x2(m[2], m[3]),
                                                                pack_bf16x2(m[4], m[5]), pack_bf16x2(m[6], m[7]));
    } else {
      float gv[8];
      Vec16<bf16>::unpack(*vec_at(g, b, oy, ox, c), gv);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = am[e] == k ? gv[e] : 0.f;
        *const_cast<uint4*>(vec_at(gx, b, 2 * oy + (k >> 1), 2 * ox + (k & 1), c)) =
            make_uint4(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7]));
      }
    }
  }
}

// ------------------------------------------------------------------ input normalisation
// h = ((v * 0.5 + 0.5) - mean_c) / std_c, evaluated in fp64 from the fp32 input and rounded once to fp32 and once to
// bf16; channels 3..7 of the 8-channel pixel are zero.
__constant__ double VGG_MEAN[3] = {0.485, 0.456, 0.406};
__constant__ double VGG_STD[3] = {0.229, 0.224, 0.225};

__global__ void vgg_norm_fwd_kernel(int B, int H, int W, const float* src, long long sb, long long sc, long long sh,
                                    long long sw, View dst) {
  const long long total = (long long)B * H * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const long long r = i / W;
    const int y = (int)(r % H), b = (int)(r / H);
    const float* s = src + b * sb + y * sh + x * sw;
    float h[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c] = (float)((((double)s[c * sc] * 0.5 + 0.5) - VGG_MEAN[c]) / VGG_STD[c]);
    *const_cast<uint4*>(vec_at(dst, b, y, x, 0)) = make_uint4(pack_bf16x2(h[0], h[1]), pack_bf16x2(h[2], 0.f), 0u, 0u);
  }
}

// dst[b][c][y][x] (fp32, contiguous) = g[b][y][x][c] * (float)(0.5 / std_c)
__global__ void vgg_norm_bwd_kernel(int B, int H, int W, View g, float* dst) {
  const long long total = (long long)B * H * W;
  const float k0 = (float)(0.5 / VGG_STD[0]), k1 = (float)(0.5 / VGG_STD[1]), k2 = (float)(0.5 / VGG_STD[2]);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const long long r = i / W;
    const int y = (int)(r % H), b = (int)(r / H);
    float gv[8];
    Vec16<bf16>::unpack(*vec_at(g, b, y, x, 0), gv);
    float* d = dst + ((long long)b * 3 * H + y) * W + x;
    const long long plane = (long long)H * W;
    d[0] = gv[0] * k0;
    d[plane] = gv[1] * k1;
    d[2 * plane] = gv[2] * k2;
  }
}

// ------------------------------------------------------------------ feature MSE
// Two-level sum in the style of stc_loss_fwd: a block of 256 threads takes 4096 elements, a thread two 8-element
// vectors (block-strided) summed in element order in fp32 (16 additions), then a binary tree over the block (8
// levels): the longest chain of fp32 additions is FMSE_CHAIN = 24; the per-block partials are summed in fp64.
constexpr int FMSE_PER_BLOCK = 4096, FMSE_CHAIN = 24;

__global__ void feat_mse_partial_kernel(const uint4* fp, const uint4* ft, long long nvec, float* part) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const long long i = (long long)blockIdx.x * 512 + k * 256 + threadIdx.x;
    if (i < nvec) {
      float a[8], b[8];
      Vec16<bf16>::unpack(fp[i], a);
      Vec16<bf16>::unpack(ft[i], b);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = a[e] - b[e];
        acc += d * d;
      }
    }
  }
  __shared__ float red[256];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ void feat_mse_final_kernel(const float* part, int nparts, long long n, float* out) {
  __shared__ double red[256];
  double a = 0;
  for (int k = threadIdx.x; k < nparts; k += 256) a += part[k];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(red[0] / (double)n);
}

// g = bf16(gout * 2 (fp - ft) / n) (fp64 product, one rounding to fp32, one to bf16), times [fp > 0] with relu_mask
__global__ void feat_mse_bwd_kernel(const uint4* fp, const uint4* ft, long long nvec, long long n, const float* gout,
                                    int relu_mask, uint4* g) {
  const double s = (double)gout[0] * 2.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
    float a[8], b[8], o[8];
    Vec16<bf16>::unpack(fp[i], a);
    Vec16<bf16>::unpack(ft[i], b);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      o[e] = (float)(s * ((double)a[e] - (double)b[e]) / (double)n);
      if (relu_mask && !(a[e] > 0.f)) o[e] = 0.f;
    }
    g[i] = make_uint4(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7]));
  }
}

static int vgg_check_view(const char* who, const char* name, const stc_view& v, int H, int W) {
  STC_REQUIRE(v.p != nullptr, "%s: %s view is NULL", who, name);
  STC_REQUIRE(v.H == H && v.W == W, "%s: %s view is %d x %d, expected %d x %d", who, name, v.H, v.W, H, W);
  STC_REQUIRE(v.cs == 1 && v.co >= 0 && v.co % 8 == 0 && v.ps >= 8 && v.ps % 8 == 0 && v.rs % 8 == 0 && v.bs % 8 == 0 &&
                  (uintptr_t)v.p % 16 == 0,
              "%s: %s view must be NHWC bf16 with 16-byte aligned pixels (cs=%d co=%d ps=%d)", who, name, v.cs, v.co,
              v.ps);
  return 0;
}

}  // namespace stc

using namespace stc;

extern "C" int stc_conv3_pack(int n, const stc_conv3_pack_desc* descs, void* stream) {
  STC_REQUIRE(n >= 1 && n <= STC_CONV3_PACK_MAX, "stc_conv3_pack: n=%d outside 1..%d", n, STC_CONV3_PACK_MAX);
  STC_REQUIRE(descs != nullptr, "stc_conv3_pack: descs is NULL");
  Pack3Args a{};
  long long most = 0;
  for (int k = 0; k < n; ++k) {
    const stc_conv3_pack_desc& d = descs[k];
    STC_REQUIRE(d.W != nullptr && (d.fwd != nullptr || d.dgrad != nullptr), "stc_conv3_pack: layer %d: NULL weight or no output", k);
    STC_REQUIRE(d.Co >= 1 && d.Ci >= 1 && d.Co_pad >= d.Co && d.Ci_pad >= d.Ci && d.Co_pad % 8 == 0 && d.Ci_pad % 8 == 0,
                "stc_conv3_pack: layer %d: Co=%d Ci=%d padded to %d, %d (multiples of 8, not smaller)", k, d.Co, d.Ci,
                d.Co_pad, d.Ci_pad);
    a.d[k] = d;
    most = std::max(most, 18ll * d.Co_pad * d.Ci_pad);
  }
  hipLaunchKernelGGL(pack3_kernel, dim3((unsigned)std::min<long long>((most + 255) / 256, 4096), (unsigned)n), dim3(256), 0,
                     (hipStream_t)stream, a);
  STC_CHECK_LAUNCH();
  return 0;
}

static int pool_check(const char* who, int B, int C, const stc_view& x, const stc_view& y) {
  STC_REQUIRE(B >= 1 && C >= 8 && C % 8 == 0, "%s: B=%d C=%d (C must be a multiple of 8)", who, B, C);
  STC_REQUIRE(x.H >= 2 && x.W >= 2 && x.H % 2 == 0 && x.W % 2 == 0, "%s: input %d x %d must be even", who, x.H, x.W);
  if (int rc = vgg_check_view(who, "input", x, x.H, x.W)) return rc;
  return vgg_check_view(who, "output", y, x.H / 2, x.W / 2);
}

extern "C" int stc_maxpool2_fwd(int B, stc_view x, int C, stc_view y, void* stream) {
  if (int rc = pool_check("stc_maxpool2_fwd", B, C, x, y)) return rc;
  const long long total = (long long)B * (x.H / 2) * (x.W / 2) * (C / 8);
  hipLaunchKernelGGL(pool2_kernel<false>, dim3(vgg_grid(total)), dim3(256), 0, (hipStream_t)stream, B, x.H / 2, x.W / 2,
                     C / 8, mkview(x), mkview(y), View{}, View{});
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_maxpool2_bwd(int B, stc_view x, int C, stc_view gy, stc_view gx, void* stream) {
  if (int rc = pool_check("stc_maxpool2_bwd", B, C, x, gy)) return rc;
  if (int rc = vgg_check_view("stc_maxpool2_bwd", "input gradient", gx, x.H, x.W)) return rc;
  const long long total = (long long)B * (x.H / 2) * (x.W / 2) * (C / 8);
  hipLaunchKernelGGL(pool2_kernel<true>, dim3(vgg_grid(total)), dim3(256), 0, (hipStream_t)stream, B, x.H / 2, x.W / 2,
                     C / 8, mkview(x), View{}, mkview(gy), mkview(gx));
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_vgg_norm_fwd(int B, int H, int W, const float* src, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                                stc_view dst, void* stream) {
  STC_REQUIRE(B >= 1 && H >= 1 && W >= 1, "stc_vgg_norm_fwd: B=%d H=%d W=%d must be >= 1", B, H, W);
  STC_REQUIRE(src != nullptr, "stc_vgg_norm_fwd: source is NULL");
  STC_REQUIRE(sb >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "stc_vgg_norm_fwd: negative source stride");
  if (int rc = vgg_check_view("stc_vgg_norm_fwd", "output", dst, H, W)) return rc;
  hipLaunchKernelGGL(vgg_norm_fwd_kernel, dim3(vgg_grid((long long)B * H * W)), dim3(256), 0, (hipStream_t)stream, B, H, W,
                     src, (long long)sb, (long long)sc, (long long)sh, (long long)sw, mkview(dst));
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_vgg_norm_bwd(int B, int H, int W, stc_view g, float* dst, void* stream) {
  STC_REQUIRE(B >= 1 && H >= 1 && W >= 1, "stc_vgg_norm_bwd: B=%d H=%d W=%d must be >= 1", B, H, W);
  STC_REQUIRE(dst != nullptr, "stc_vgg_norm_bwd: destination is NULL");
  if (int rc = vgg_check_view("stc_vgg_norm_bwd", "gradient", g, H, W)) return rc;
  hipLaunchKernelGGL(vgg_norm_bwd_kernel, dim3(vgg_grid((long long)B * H * W)), dim3(256), 0, (hipStream_t)stream, B, H, W,
                     mkview(g), dst);
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_feat_mse_parts(int64_t n) { return (int)((n + FMSE_PER_BLOCK - 1) / FMSE_PER_BLOCK); }
extern "C" int stc_feat_mse_chain(void) { return FMSE_CHAIN; }

static int fmse_check(const char* who, const void* fp, const void* ft, int64_t n) {
  STC_REQUIRE(fp != nullptr && ft != nullptr, "%s: feature tensor is NULL", who);
  STC_REQUIRE(n > 0 && n % 8 == 0, "%s: n=%lld must be a positive multiple of 8", who, (long long)n);
  STC_REQUIRE((uintptr_t)fp % 16 == 0 && (uintptr_t)ft % 16 == 0, "%s: feature tensors must be 16-byte aligned", who);
  return 0;
}

extern "C" int stc_feat_mse_fwd(const void* fp, const void* ft, int64_t n, float* part, float* out, void* stream) {
  if (int rc = fmse_check("stc_feat_mse_fwd", fp, ft, n)) return rc;
  STC_REQUIRE(part != nullptr, "stc_feat_mse_fwd: workspace (stc_feat_mse_parts floats) is NULL");
  STC_REQUIRE(out != nullptr, "stc_feat_mse_fwd: out is NULL");
  const int np = stc_feat_mse_parts(n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(feat_mse_partial_kernel, dim3(np), dim3(256), 0, st, (const uint4*)fp, (const uint4*)ft,
                     (long long)(n / 8), part);
  STC_CHECK_LAUNCH();
  hipLaunchKernelGGL(feat_mse_final_kernel, dim3(1), dim3(256), 0, st, (const float*)part, np, (long long)n, out);
  STC_CHECK_LAUNCH();
  return 0;
}

extern "C" int stc_feat_mse_bwd(const void* fp, const void* ft, int64_t n, const float* gout, int relu_mask, void* g,
                                void* stream) {
  if (int rc = fmse_check("stc_feat_mse_bwd", fp, ft, n)) return rc;
  STC_REQUIRE(gout != nullptr && g != nullptr && (uintptr_t)g % 16 == 0, "stc_feat_mse_bwd: gout / g NULL or unaligned");
  hipLaunchKernelGGL(feat_mse_bwd_kernel, dim3(vgg_grid(n / 8)), dim3(256), 0, (hipStream_t)stream, (const uint4*)fp,
                     (const uint4*)ft, (long long)(n / 8), (long long)n, gout, relu_mask ? 1 : 0, (uint4*)g);
  STC_CHECK_LAUNCH();
  return 0;
}
