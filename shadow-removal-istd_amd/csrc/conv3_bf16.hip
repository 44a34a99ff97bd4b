// bf16 Conv2d k3 s1 p1 as an implicit GEMM whose A operand is an LDS-resident input halo (gfx950).
//
// The VGG-19-bn feature convolutions of VisualLoss (src/loss.py:29-56 of the reference's src/ line; the
// torchvision vgg19_bn `features` Sequential), forward and input gradient: y = relu(conv3x3(x, w) + b), and with the
// weights packed for it (taps flipped, ci / co swapped: stc_conv3_pack) dx = conv3x3(dy, w^T) * [a > 0].
//
// A block owns a 16 x 16 patch of output pixels of one image (BM = 256 GEMM rows) and 64 output channels.  Per
// 32-channel chunk of the input it stages
//   A: the 18 x 18 input halo of the patch, one 64-byte LDS row per pixel (position P = hr * 18 + hc holds input
//      pixel (y0 + hr - 1, x0 + hc - 1)); pixels outside the image -- the zero padding -- and channels past Cin are
//      LDS-DMA pieces with an out-of-range offset, which land as zeros: no padded copy of the tensor exists;
//   B: the 9 taps x 64 output channels x 32 input channels of the packed weights [Cout][9][Cin], one 64-byte LDS row
//      per (tap, n),
// so every staged pixel serves all 9 taps (an im2col tile would stage it 9 times), as halo_bf16.hip does for k4.
// Tap (ky, kx) of the 16 pixels of patch row r is the A fragment at positions (r + ky) * 18 + kx + [0, 16): 16
// consecutive LDS rows from an arbitrary first row, conflict-free under halo_bf16.hip's 64-byte-row swizzle.
// 4 waves, each 4 patch rows x 64 channels (16 accumulator tiles of v_mfma_f32_16x16x32_bf16); 60 KiB of LDS, so two
// blocks share a CU and one block's stage wait overlaps the other's MFMAs (the stage itself is not double-buffered).
// K order: 32-channel chunk -> ky -> kx -> the MFMA's own: fixed, no split, no atomics -- bit-identical run to run.
// Epilogue: + bias[n], ReLU, one rounding to bf16, through LDS to 16-byte NHWC stores; the input-gradient form
// multiplies by [a > 0] of a second view at the same pixel and channel instead.
#include "igemm_bf16.hpp"

namespace stc {

constexpr int C3_TH = 16, C3_TW = 16, C3_BM = C3_TH * C3_TW, C3_BN = 64, C3_KC = 32;
constexpr int C3_HP = C3_TW + 2;                 // halo pitch, pixels
constexpr int C3_AP = 24;                        // 16-pixel (1 KiB) DMA pieces of the A stage: 384 >= 18 * 18 positions
constexpr int C3_A = C3_AP * 1024, C3_B = 9 * C3_BN * 64;
constexpr int C3_LDS = C3_A + C3_B;              // 60 KiB
constexpr int C3_PITCH = C3_BN * 2 + 16;         // epilogue tile row, bytes
static_assert(C3_BM * C3_PITCH <= C3_LDS, "epilogue tile");
static_assert((C3_TH + 2) * C3_HP <= C3_AP * 16, "halo positions");

struct C3Params {
  const char* a;
  unsigned a_bytes;
  int a_bs, a_rs, a_ps, a_co;  // elements (a_bytes < 2^31)
  const char* b;
  unsigned b_bytes;
  int H, W, cin, N;
  int tx, ty, ntiles;  // patches per row / column of an image, N tiles
  char* c;
  long long c_bs, c_rs;
  int c_ps, c_co;
  const float* bias;
  int relu;
  const char* m;  // optional mask view a: out *= [a > 0]
  long long m_bs, m_rs;
  int m_ps, m_co;
};

__device__ __forceinline__ int c3_swz(int row) { return ((row >> 2) & 1) << 1; }

// out = a > 0 ? v : 0 per bf16 element
__device__ __forceinline__ unsigned c3_mask2(unsigned v, unsigned a) {
  const unsigned lo = __uint_as_float(a << 16) > 0.f ? 0x0000ffffu : 0u;
  const unsigned hi = __uint_as_float(a & 0xffff0000u) > 0.f ? 0xffff0000u : 0u;
  return v & (lo | hi);
}

__global__ void __launch_bounds__(256, 2) conv3_kernel(const C3Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sA = smem;
  char* sB = smem + C3_A;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // consecutive blocks: the N tiles of one patch (the same halo), then the patches along a row
  int bid = blockIdx.x;
  const int nt = bid % p.ntiles;
  bid /= p.ntiles;
  const int txi = bid % p.tx;
  bid /= p.tx;
  const int tyi = bid % p.ty, img = bid / p.ty;
  const int y0 = tyi * C3_TH, x0 = txi * C3_TW, n0 = nt * C3_BN;

  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)p.a, (short)0, (int)p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)p.b, (short)0, (int)p.b_bytes, 0x00020000);

  // ---- DMA lane roles: lane -> (row prow of its 16-row piece, LDS slot lane & 3 <- source chunk schunk)
  constexpr int AG = C3_AP / 4, BG = 9;  // pieces per wave and stage
  const int prow = lane >> 2;
  const int schunk = (lane & 3) ^ c3_swz(prow);  // (pieces are 16-row aligned: swz(position) == swz(prow))
  unsigned a_off[AG], b_off[BG];
#pragma unroll
  for (int g = 0; g < AG; ++g) {
    const int pos = (wave * AG + g) * 16 + prow;
    const int hr = pos / C3_HP, hc = pos - hr * C3_HP;
    const int iy = y0 + hr - 1, ix = x0 + hc - 1;
    const bool ok = hr < C3_TH + 2 && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    a_off[g] = ok ? (unsigned)(img * p.a_bs + iy * p.a_rs + ix * p.a_ps + p.a_co + schunk * 8) : OOB;
  }
#pragma unroll
  for (int h = 0; h < BG; ++h) {
    const int q = wave * BG + h;  // piece q = rows [16 q, 16 q + 16) of the stage: tap q / 4, channels 16 (q & 3) ..
    const int tap = q >> 2, n = n0 + (q & 3) * 16 + prow;
    b_off[h] = n < p.N ? (unsigned)((n * 9 + tap) * p.cin + schunk * 8) : OOB;
  }

  constexpr int FM = 4, FN = 4;
  floatx4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int rl = lane & 15, kq = lane >> 4;
  const int b_rd = rl * 64 + ((kq ^ c3_swz(rl)) * 16);

  for (int c0 = 0; c0 < p.cin; c0 += C3_KC) {
    const unsigned cpen = c0 + schunk * 8 < p.cin ? 0u : OOB;  // channels past Cin: zeros
#pragma unroll
    for (int g = 0; g < AG; ++g)
      dma16(ra, sA + (wave * AG + g) * 1024, ((a_off[g] + (unsigned)c0) * 2u) | (a_off[g] & OOB) | cpen);
#pragma unroll
    for (int h = 0; h < BG; ++h)
      dma16(rb, sB + (wave * BG + h) * 1024, ((b_off[h] + (unsigned)c0) * 2u) | (b_off[h] & OOB) | cpen);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // every wave's pieces landed
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        bf16x8_t fa[FM], fb[FN];
#pragma unroll
        for (int j = 0; j < FN; ++j)
          fb[j] = *reinterpret_cast<const bf16x8_t*>(sB + ((ky * 3 + kx) * C3_BN + j * 16) * 64 + b_rd);
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const int P = (wave * FM + i + ky) * C3_HP + kx + rl;
          fa[i] = *reinterpret_cast<const bf16x8_t*>(sA + P * 64 + ((kq ^ c3_swz(P)) * 16));
        }
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) acc[i][j] = exp_mfma(fa[i], fb[j], acc[i][j]);
      }
    __syncthreads();  // every wave done with the stage
  }

  // ---- epilogue: accumulator element (i, j, r) = patch row wave * 4 + i, column 4 * (lane >> 4) + r, channel 16 j + rl
  const int rq = 4 * kq;
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int n = n0 + 16 * j + rl;
    const float bz = p.bias && n < p.N ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[i][j][r] + bz;
        if (p.relu) v = v > 0.f ? v : 0.f;
        const int pix = (wave * FM + i) * C3_TW + rq + r;
        *reinterpret_cast<unsigned short*>(smem + pix * C3_PITCH + (16 * j + rl) * 2) = f2bf(v);
      }
  }
  __syncthreads();
  constexpr int ITER = C3_BM * (C3_BN / 8) / 256;
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int idx = tid + it * 256;
    const int pix = idx >> 3, cc = idx & 7;
    const int y = y0 + (pix >> 4), x = x0 + (pix & 15), n = n0 + cc * 8;
    if (y >= p.H || x >= p.W || n >= p.N) continue;
    uint4 v = *reinterpret_cast<const uint4*>(smem + pix * C3_PITCH + cc * 16);
    if (p.m) {
      const uint4 a = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(p.m) + (long long)img * p.m_bs +
                                                      (long long)y * p.m_rs + (long long)x * p.m_ps + p.m_co + n);
      v = make_uint4(c3_mask2(v.x, a.x), c3_mask2(v.y, a.y), c3_mask2(v.z, a.z), c3_mask2(v.w, a.w));
    }
    *reinterpret_cast<uint4*>(reinterpret_cast<bf16*>(p.c) + (long long)img * p.c_bs + (long long)y * p.c_rs +
                              (long long)x * p.c_ps + p.c_co + n) = v;
  }
}

static int c3_check_shape(const char* who, int B, int H, int W, int Cin, int Cout) {
  STC_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: B=%d H=%d W=%d must be >= 1", who, B, H, W);
  STC_REQUIRE((long long)B * H * W < (1ll << 24), "%s: B*H*W = %lld must be < 2^24", who, (long long)B * H * W);
  STC_REQUIRE(Cin >= 8 && Cin % 8 == 0, "%s: Cin=%d must be a multiple of 8 (store a 3-channel input as 8)", who, Cin);
  STC_REQUIRE(Cout >= 8 && Cout % 8 == 0, "%s: Cout=%d must be a multiple of 8", who, Cout);
  STC_REQUIRE(9ll * Cin * Cout * 2 < (1ll << 31), "%s: packed weight of Cin=%d Cout=%d exceeds 2 GiB", who, Cin, Cout);
  return 0;
}

static int c3_check_view(const char* who, const char* name, const stc_view& v, int H, int W) {
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

extern "C" int stc_conv3_plan(int B, int H, int W, int Cin, int Cout, int32_t* out) {
  if (int rc = c3_check_shape("stc_conv3_plan", B, H, W, Cin, Cout)) return rc;
  STC_REQUIRE(out != nullptr, "stc_conv3_plan: out is NULL");
  const int tx = cdiv(W, C3_TW), ty = cdiv(H, C3_TH);
  out[0] = 0;  // path: the one halo kernel (no first-layer path of its own)
  out[1] = C3_TH;
  out[2] = C3_TW;
  out[3] = C3_BN;
  out[4] = C3_KC;
  out[5] = 1;  // K splits
  out[6] = B * ty * tx;
  out[7] = cdiv(Cout, C3_BN);
  return 0;
}

extern "C" int stc_conv3_fwd(int B, stc_view x, int Cin, const void* w_packed, int Cout, stc_view y,
                             const float* bias, int relu, stc_view mask, void* stream) {
  if (int rc = c3_check_shape("stc_conv3_fwd", B, x.H, x.W, Cin, Cout)) return rc;
  const int H = x.H, W = x.W;
  if (int rc = c3_check_view("stc_conv3_fwd", "input", x, H, W)) return rc;
  if (int rc = c3_check_view("stc_conv3_fwd", "output", y, H, W)) return rc;
  if (mask.p)
    if (int rc = c3_check_view("stc_conv3_fwd", "mask", mask, H, W)) return rc;
  STC_REQUIRE(w_packed != nullptr, "stc_conv3_fwd: packed weight is NULL");
  STC_REQUIRE(x.bs >= 0 && x.rs >= 0 && x.ps >= 8 && y.bs >= 0 && y.rs >= 0 && y.ps >= 8,
              "stc_conv3_fwd: negative or sub-vector strides");
  const long long a_elems = (long long)(B - 1) * x.bs + (long long)(H - 1) * x.rs + (long long)(W - 1) * x.ps + x.co + Cin;
  STC_REQUIRE(a_elems * 2 < (1ll << 31), "stc_conv3_fwd: input extent %lld bytes exceeds 2 GiB", a_elems * 2);
  C3Params p{};
  p.a = (const char*)x.p;
  p.a_bytes = (unsigned)(a_elems * 2);
  p.a_bs = (int)x.bs; p.a_rs = (int)x.rs; p.a_ps = x.ps; p.a_co = x.co;
  p.b = (const char*)w_packed;
  p.b_bytes = (unsigned)(9ll * Cin * Cout * 2);
  p.H = H; p.W = W; p.cin = Cin; p.N = Cout;
  p.tx = cdiv(W, C3_TW); p.ty = cdiv(H, C3_TH); p.ntiles = cdiv(Cout, C3_BN);
  p.c = (char*)y.p;
  p.c_bs = y.bs; p.c_rs = y.rs; p.c_ps = y.ps; p.c_co = y.co;
  p.bias = bias;
  p.relu = relu ? 1 : 0;
  p.m = (const char*)mask.p;
  p.m_bs = mask.bs; p.m_rs = mask.rs; p.m_ps = mask.ps; p.m_co = mask.co;
  const long long blocks = (long long)B * p.ty * p.tx * p.ntiles;
  STC_REQUIRE(blocks < (1ll << 31), "stc_conv3_fwd: %lld blocks", blocks);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(conv3_kernel, dim3((unsigned)blocks), dim3(256), C3_LDS, st, p);
  STC_CHECK_LAUNCH();
  return 0;
}
