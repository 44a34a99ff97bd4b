// The body of smalln_kernel and smalln_reflect_kernel (igemm.hip): see igemm_tile.inc.
  constexpr int VEC = 16 / sizeof(T);
  constexpr int NMAX = 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* wl = reinterpret_cast<T*>(smem);  // [N][K] of this phase
  const int ph = blockIdx.y;
  const T* wsrc = reinterpret_cast<const T*>(p.b) + p.b_phase_stride * ph;
  const int NK = p.N * p.K;
  for (int i = threadIdx.x * VEC; i < NK; i += 256 * VEC)
    *reinterpret_cast<uint4*>(wl + i) = *reinterpret_cast<const uint4*>(wsrc + i);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunks = p.K / VEC;
  const int GHW = p.GH * p.GW;
  const int tw_mask = (1 << p.lg_tw) - 1;
  const int offy = p.offy[ph], offx = p.offx[ph];
  const T* A = reinterpret_cast<const T*>(p.a);
  for (int m = blockIdx.x * 4 + wave; m < p.M; m += gridDim.x * 4) {
    const int b = m / GHW, rem = m - b * GHW;
    const int y = rem / p.GW, x = rem - y * p.GW;
    const long long abase = (long long)b * p.a_bs + p.a_co;
    float acc[NMAX];
#pragma unroll
    for (int n = 0; n < NMAX; ++n) acc[n] = 0.f;
    for (int c = lane; c < nchunks; c += 64) {
      const int k = c * VEC;
      const int t = k / p.cin, ci = k - t * p.cin;
      int iy = y * p.in_stride + offy + p.stepy * (t >> p.lg_tw);
      int ix = x * p.in_stride + offx + p.stepx * (t & tw_mask);
      STC_HALO_REMAP(iy, ix, p.IH, p.IW)
      if ((unsigned)iy >= (unsigned)p.IH || (unsigned)ix >= (unsigned)p.IW) continue;
      uint4 v = *reinterpret_cast<const uint4*>(A + abase + (long long)iy * p.a_rs + (long long)ix * p.a_ps + ci);
      if (p.sc || p.pro_act) v = prologue16<T>(v, p.sc, p.sh, ci, p.pro_act, p.slope);
      float av[VEC];
      if constexpr (sizeof(T) == 4) {
        av[0] = __uint_as_float(v.x); av[1] = __uint_as_float(v.y);
        av[2] = __uint_as_float(v.z); av[3] = __uint_as_float(v.w);
      } else {
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) { av[2 * q] = __uint_as_float(w[q] << 16); av[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u); }
      }
#pragma unroll
      for (int n = 0; n < NMAX; ++n) {
        if (n >= p.N) break;
        const T* wr = wl + n * p.K + k;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[n] = fmaf(av[e], ld1<T>(wr + e), acc[n]);
      }
    }
#pragma unroll
    for (int n = 0; n < NMAX; ++n) {
      if (n >= p.N) break;
      float s = acc[n];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      acc[n] = s;
    }
    if (lane < p.N) {
      float v = 0.f;
#pragma unroll
      for (int n = 0; n < NMAX; ++n) if (n == lane) v = acc[n];
      if (p.bias) v += p.bias[lane];
      v = head_act(v, p.tanh_);
      const int oy = y * p.os + p.oy0[ph], ox = x * p.os + p.ox0[ph];
      const long long off = (long long)b * p.c_bs + (long long)oy * p.c_rs + (long long)ox * p.c_ps +
                            (long long)(p.c_co + lane) * p.c_cs;
      if (p.out_f32) reinterpret_cast<float*>(p.c)[off] = v;
      else st1<T>(reinterpret_cast<T*>(p.c) + off, v);
    }
  }
