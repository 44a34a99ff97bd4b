// The 16-byte channel vector of the NHWC kernels: 4 fp32 or 8 bf16 consecutive channels per thread
// (bn.hip, inorm.hip, vgg.hip), as the raw uint4 and as N floats.
#pragma once
#include "common.hpp"

namespace stc {

template <typename T> struct Vec16 {
  static constexpr int N = 16 / (int)sizeof(T);
  static_assert(N == 4 || N == 8, "Vec16: float or bf16");
  __device__ __forceinline__ static uint4 ldraw(const T* p) { return *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ static void straw(T* p, const uint4& v) { *reinterpret_cast<uint4*>(p) = v; }
  __device__ __forceinline__ static void unpack(const uint4& v, float* f) {
    if constexpr (N == 4) {
      f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
    } else {
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) { f[2 * q] = __uint_as_float(w[q] << 16); f[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u); }
    }
  }
  __device__ __forceinline__ static uint4 pack(const float* f) {  // bf16: round-to-nearest-even (f2bf)
    if constexpr (N == 4) {
      return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
    } else {
      uint4 v;
      v.x = (unsigned)f2bf(f[0]) | ((unsigned)f2bf(f[1]) << 16);
      v.y = (unsigned)f2bf(f[2]) | ((unsigned)f2bf(f[3]) << 16);
      v.z = (unsigned)f2bf(f[4]) | ((unsigned)f2bf(f[5]) << 16);
      v.w = (unsigned)f2bf(f[6]) | ((unsigned)f2bf(f[7]) << 16);
      return v;
    }
  }
  __device__ __forceinline__ static void load(const T* p, float* f) { unpack(ldraw(p), f); }
  __device__ __forceinline__ static void store(T* p, const float* f) { straw(p, pack(f)); }
};

// N (a multiple of 4) consecutive fp32 table entries
template <int N>
__device__ __forceinline__ void ldc(const float* p, float* f) {
#pragma unroll
  for (int e = 0; e < N; e += 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + e);
    f[e] = v.x; f[e + 1] = v.y; f[e + 2] = v.z; f[e + 3] = v.w;
  }
}

}  // namespace stc
