// The generator's dropout mask (use_dropout=True: STCGAN/networks.py UnetSkipConnectionBlock, nn.Dropout after the
// up-norm) as a pure function of logical indices -- the one definition every dropout kernel uses (forward apply,
// BatchNorm backward, mask export), so that fp32, bf16, every stream schedule and a CPU restatement agree bit for bit.
//
//   Philox4x32-10 (Random123 constants; counter = key = 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8)
//   key     = the 64-bit seed (lo, hi)
//   counter = (idx >> 2, level, offset lo, offset hi)
//             idx: the element's NHWC linear index over the full ConvT extent (B, H, W, C), idx < 2^34;
//             level: the U-Net block whose up-norm output is dropped; offset: the per-call counter
//   element idx uses output word idx & 3;  keep <=> word >= floor(p * 2^32) (unsigned);  kept values * 1/(1-p) (fp32)
//
// {seed, offset} are read from device memory (the per-call copy stc_dropout_next makes), never baked into a launch:
// a replayed HIP graph draws a fresh mask each time.
#pragma once
#include <stdint.h>

#include "common.hpp"

namespace stc {

struct DropDev {  // device-side copy of stc_dropout
  const unsigned long long* state;  // {seed, offset} of this call
  unsigned level, thresh;
  float scale;
  int H, W;  // full extent the logical index runs over
};

struct DropKey {  // the call's {seed, offset}, loaded once per thread
  unsigned k0, k1, o0, o1;
};
__device__ __forceinline__ DropKey drop_key(const DropDev& d) {
  const unsigned long long seed = d.state[0], off = d.state[1];
  return DropKey{(unsigned)seed, (unsigned)(seed >> 32), (unsigned)off, (unsigned)(off >> 32)};
}

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned* out) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const unsigned hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// logical NHWC index of (b, y, x, c) over the full extent
__device__ __forceinline__ unsigned long long drop_index(const DropDev& d, int C, int b, int y, int x, int c) {
  return (((unsigned long long)b * d.H + y) * d.W + x) * (unsigned long long)C + c;
}

// keep[e] (0 / 1) of the 4 elements idx .. idx + 3 (idx % 4 == 0): one Philox call
__device__ __forceinline__ void drop_keep4(const DropDev& d, const DropKey& k, unsigned long long idx, unsigned* keep) {
  unsigned w[4];
  philox4x32_10((unsigned)(idx >> 2), d.level, k.o0, k.o1, k.k0, k.k1, w);
#pragma unroll
  for (int e = 0; e < 4; ++e) keep[e] = w[e] >= d.thresh ? 1u : 0u;
}

// m[e] = keep ? 1/(1-p) : 0 for the N (4 or 8) channels starting at logical index idx (idx % 4 == 0)
template <int N>
__device__ __forceinline__ void drop_factor(const DropDev& d, const DropKey& k, unsigned long long idx, float* m) {
#pragma unroll
  for (int q = 0; q < N; q += 4) {
    unsigned keep[4];
    drop_keep4(d, k, idx + q, keep);
#pragma unroll
    for (int e = 0; e < 4; ++e) m[q + e] = keep[e] ? d.scale : 0.f;
  }
}

}  // namespace stc
