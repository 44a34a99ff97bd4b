// The body of igemm_kernel and igemm_reflect_kernel (igemm.hip), included once into each: T, BM, BN, WM, WN, PRO and
// p are the including kernel's.  STC_HALO_REMAP(iy, ix, IH, IW) is empty for the zero-filled halo and the reflect map
// for the reflected one -- the only difference between the two kernels (an inlined template body scheduled the
// existing kernels differently; the same text compiles to the same code).
  constexpr int VEC = 16 / sizeof(T);
  constexpr int BK = 128 / sizeof(T);
  constexpr int AIT = BM / 32;  // 16-byte chunks per thread for A (8 chunks per row)
  constexpr int BIT = BN / 32;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int FM = WTM / 32, FN = WTN / 32;
  constexpr int STAGE = (BM + BN) * LDS_ROW;
  static_assert(WM * WN == 4, "4 waves");
  static_assert(FM >= 1 && FN >= 1, "wave tile >= 32x32");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  long long* rowoff = reinterpret_cast<long long*>(smem + 2 * STAGE);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;

  // XCD-aware bijective remap of the flat tile id: consecutive tiles (sharing A rows)
  // land on the same XCD's L2.
  const int nwg = p.mtiles * p.ntiles;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int mt = bid / p.ntiles, nt = bid % p.ntiles;
  const int m0 = mt * BM, n0 = nt * BN;
  const int z = blockIdx.z;
  const int ph = z / p.ksplit, split = z % p.ksplit;
  const int kbeg = split * p.kchunk;
  const int kend = min(p.K, kbeg + p.kchunk);
  const int nsteps = (kend - kbeg + BK - 1) / BK;  // a partial last step is zero-filled past kend
  const int GHW = p.GH * p.GW;
  const int offy = p.offy[ph], offx = p.offx[ph];
  const int tw_mask = (1 << p.lg_tw) - 1;

  // ---- per-thread A row info
  const int ca = tid & 7;
  long long abase[AIT];
  int ayy[AIT], axx[AIT];
#pragma unroll
  for (int i = 0; i < AIT; ++i) {
    const int m = m0 + (tid >> 3) + 32 * i;
    if (m < p.M) {
      const int b = m / GHW, rem = m - b * GHW;
      const int y = rem / p.GW, x = rem - y * p.GW;
      abase[i] = (long long)b * p.a_bs + p.a_co;
      ayy[i] = y * p.in_stride + offy;
      axx[i] = x * p.in_stride + offx;
    } else {
      abase[i] = 0;
      ayy[i] = -100000;  // always out of bounds
      axx[i] = -100000;
    }
  }
  // ---- per-thread B row info
  const T* bptr[BIT];
  bool bval[BIT];
#pragma unroll
  for (int j = 0; j < BIT; ++j) {
    const int n = n0 + (tid >> 3) + 32 * j;
    bval[j] = n < p.N;
    bptr[j] = reinterpret_cast<const T*>(p.b) + p.b_phase_stride * ph + (long long)(bval[j] ? n : 0) * p.K + ca * VEC;
  }
  // ---- output row offsets (direct epilogue)
  if (!p.ws) {
    for (int r = tid; r < BM; r += 256) {
      const int m = m0 + r;
      long long off = -1;
      if (m < p.M) {
        const int b = m / GHW, rem = m - b * GHW;
        const int y = rem / p.GW, x = rem - y * p.GW;
        const int oy = y * p.os + p.oy0[ph], ox = x * p.os + p.ox0[ph];
        off = (long long)b * p.c_bs + (long long)oy * p.c_rs + (long long)ox * p.c_ps;
      }
      rowoff[r] = off;
    }
  }

  // Two register staging sets (ping-pong): the global loads of K-step s+2 are issued at
  // step s and written to LDS at the end of step s+1, so two steps of MFMA work cover
  // their latency (a bf16 K-step is only 16 MFMAs per wave).
  struct Regs {
    uint4 ra[AIT], rb[BIT];
    unsigned amask;  // which A chunks were in bounds (prologue must not touch padding)
    int aci;         // channel of this thread's chunk in the staged K-step
  };
  Regs r0, r1;
  const T* abase_ptr = reinterpret_cast<const T*>(p.a);
  constexpr bool has_pro = PRO;  // the engine materialises activations: PRO=false on its hot path

  auto load_regs = [&](Regs& R, int k0) {
    const int k = k0 + ca * VEC;
    const int t = k / p.cin, ci = k - t * p.cin;
    const int dy = p.stepy * (t >> p.lg_tw), dx = p.stepx * (t & tw_mask);
    R.aci = ci;
    R.amask = 0;
    const bool kin = k < kend;
#pragma unroll
    for (int i = 0; i < AIT; ++i) {
      int iy = ayy[i] + dy, ix = axx[i] + dx;
      STC_HALO_REMAP(iy, ix, p.IH, p.IW)
      if (kin && (unsigned)iy < (unsigned)p.IH && (unsigned)ix < (unsigned)p.IW) {
        const T* src = abase_ptr + abase[i] + (long long)iy * p.a_rs + (long long)ix * p.a_ps + ci;
        R.ra[i] = *reinterpret_cast<const uint4*>(src);
        R.amask |= 1u << i;
      } else {
        R.ra[i] = make_uint4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < BIT; ++j) {
      R.rb[j] = (bval[j] && kin) ? *reinterpret_cast<const uint4*>(bptr[j] + k0) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_lds = [&](Regs& R, int stage) {
    char* sA = smem + stage * STAGE;
    char* sB = sA + BM * LDS_ROW;
#pragma unroll
    for (int i = 0; i < AIT; ++i) {
      uint4 v = R.ra[i];
      if (has_pro && (R.amask >> i & 1u)) v = prologue16<T>(v, p.sc, p.sh, R.aci, p.pro_act, p.slope);
      *reinterpret_cast<uint4*>(sA + ((tid >> 3) + 32 * i) * LDS_ROW + ca * 16) = v;
    }
#pragma unroll
    for (int j = 0; j < BIT; ++j)
      *reinterpret_cast<uint4*>(sB + ((tid >> 3) + 32 * j) * LDS_ROW + ca * 16) = R.rb[j];
  };

  floatx16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int lrow = lane & 31, lhalf = lane >> 5;
  auto compute = [&](int cur) {
    const char* sA = smem + cur * STAGE;
    const char* sB = sA + BM * LDS_ROW;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const int coff = (2 * kc + lhalf) * 16;
      uint4 fa[FM], fb[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i)
        fa[i] = *reinterpret_cast<const uint4*>(sA + (wm * WTM + 32 * i + lrow) * LDS_ROW + coff);
#pragma unroll
      for (int j = 0; j < FN; ++j)
        fb[j] = *reinterpret_cast<const uint4*>(sB + (wn * WTN + 32 * j + lrow) * LDS_ROW + coff);
      if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int i = 0; i < FM; ++i) {
            const float av = __uint_as_float(e == 0 ? fa[i].x : e == 1 ? fa[i].y : e == 2 ? fa[i].z : fa[i].w);
#pragma unroll
            for (int j = 0; j < FN; ++j) {
              const float bv = __uint_as_float(e == 0 ? fb[j].x : e == 1 ? fb[j].y : e == 2 ? fb[j].z : fb[j].w);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[i][j], 0, 0, 0);
            }
          }
        }
      } else {
        typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const bf16x8 av = __builtin_bit_cast(bf16x8, fa[i]);
#pragma unroll
          for (int j = 0; j < FN; ++j) {
            const bf16x8 bv = __builtin_bit_cast(bf16x8, fb[j]);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[i][j], 0, 0, 0);
          }
        }
      }
    }
  };

  if (nsteps > 0) {
    load_regs(r0, kbeg);
    store_lds(r0, 0);
  }
  if (nsteps > 1) load_regs(r1, kbeg + BK);
  __syncthreads();
  // step s: set (s&1) held step s (already in LDS stage s&1); set ((s+1)&1) holds step s+1
  for (int s = 0; s < nsteps; s += 2) {
    if (s + 2 < nsteps) load_regs(r0, kbeg + (s + 2) * BK);
    compute(0);
    if (s + 1 < nsteps) store_lds(r1, 1);
    __syncthreads();
    if (s + 1 >= nsteps) break;
    if (s + 3 < nsteps) load_regs(r1, kbeg + (s + 3) * BK);
    compute(1);
    if (s + 2 < nsteps) store_lds(r0, 0);
    __syncthreads();
  }

  // ---- epilogue
  if (p.ws) {
    float* slab = p.ws + (long long)z * p.M * p.N;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int n = n0 + wn * WTN + 32 * j + lrow;
        if (n >= p.N) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = m0 + wm * WTM + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
          if (m < p.M) slab[(long long)m * p.N + n] = acc[i][j][e];
        }
      }
    return;
  }
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int n = n0 + wn * WTN + 32 * j + lrow;
    if (n >= p.N) continue;
    const float bz = p.bias ? p.bias[n] : 0.f;
    const long long coff = (long long)(p.c_co + n) * p.c_cs;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = wm * WTM + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
        const long long ro = rowoff[r];
        if (ro < 0) continue;
        float v = acc[i][j][e] + bz;
        v = head_act(v, p.tanh_);
        if (p.out_f32) reinterpret_cast<float*>(p.c)[ro + coff] = v;
        else st1<T>(reinterpret_cast<T*>(p.c) + ro + coff, v);
      }
    }
  }
