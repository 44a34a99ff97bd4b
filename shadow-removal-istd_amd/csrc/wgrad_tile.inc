// The body of wgrad_kernel and wgrad_reflect_kernel (wgrad.hip), included once into each: T and p are the including
// kernel's; STC_HALO_REMAP as in igemm_tile.inc.
  constexpr int VEC = 16 / sizeof(T);
  constexpr int CPR = WG_BM * (int)sizeof(T) / 16;  // 16-byte chunks per staged row (32 fp32 / 16 bf16)
  constexpr int RPP = 256 / CPR;                     // rows per pass
  constexpr int NP = WG_BK / RPP;                    // passes per K-step (4 fp32 / 2 bf16)
  constexpr int ROWB = WgCfg<T>::ROWB;
  constexpr int TILEB = WG_BK * ROWB;
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILEB];  // [stage][A|B]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int nwg = p.mtiles * p.ntiles;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int mt = bid / p.ntiles, nt = bid % p.ntiles;
  const int r0 = mt * WG_BM, c0 = nt * WG_BN;
  const int split = blockIdx.z;
  const int pbeg = split * p.pchunk;
  const int pend = min(p.P, pbeg + p.pchunk);
  const int GHW = p.GH * p.GW;

  // staging map: row (pixel) kp = tid/CPR + RPP*i, chunk = tid%CPR (VEC channels)
  const int chunk = tid % CPR;
  const int rr = r0 + chunk * VEC;   // D channel of this chunk
  const int col = c0 + chunk * VEC;  // G column of this chunk
  const bool rval = rr < p.R;
  const bool cval = col < p.Ncol;
  const int t = col / p.Cg, ci = col - t * p.Cg;
  const int kh = t >> 2, kw = t & 3;
  const T* Dp = reinterpret_cast<const T*>(p.d);
  const T* Gp = reinterpret_cast<const T*>(p.g);
  const float* dsc = p.dsc ? p.dsc + rr : nullptr;
  const float* dsh = p.dsh ? p.dsh + rr : nullptr;
  const float* gsc = p.gsc ? p.gsc + ci : nullptr;
  const float* gsh = p.gsh ? p.gsh + ci : nullptr;
  const bool dpro = p.dsc != nullptr || p.dact;
  const bool gpro = p.gsc != nullptr || p.gact;

  uint4 va[NP], vb[NP];
  unsigned ma = 0, mb = 0;
  auto load = [&](int k0) {
    ma = 0; mb = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int pix = k0 + tid / CPR + RPP * i;
      va[i] = make_uint4(0, 0, 0, 0);
      vb[i] = make_uint4(0, 0, 0, 0);
      if (pix < pend) {
        const int b = pix / GHW, rem = pix - b * GHW;
        const int oy = rem / p.GW, ox = rem - oy * p.GW;
        if (rval) {
          va[i] = *reinterpret_cast<const uint4*>(Dp + (long long)b * p.d_bs + (long long)oy * p.d_rs +
                                                  (long long)ox * p.d_ps + p.d_co + rr);
          ma |= 1u << i;
        }
        int iy = oy * p.stride + kh - 1, ix = ox * p.stride + kw - 1;
        STC_HALO_REMAP(iy, ix, p.IH, p.IW)
        if (cval && (unsigned)iy < (unsigned)p.IH && (unsigned)ix < (unsigned)p.IW) {
          vb[i] = *reinterpret_cast<const uint4*>(Gp + (long long)b * p.g_bs + (long long)iy * p.g_rs +
                                                  (long long)ix * p.g_ps + p.g_co + ci);
          mb |= 1u << i;
        }
      }
    }
  };
  auto store = [&](int st) {
    char* sA = smem + st * 2 * TILEB;
    char* sB = sA + TILEB;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int kp = tid / CPR + RPP * i;
      uint4 a = va[i], b = vb[i];
      if (dpro && (ma >> i & 1u)) a = wg_pro<T>(a, dsc, dsh, p.dact, p.dslope);
      if (gpro && (mb >> i & 1u)) b = wg_pro<T>(b, gsc, gsh, p.gact, p.gslope);
      *reinterpret_cast<uint4*>(sA + kp * ROWB + chunk * 16) = a;
      *reinterpret_cast<uint4*>(sB + kp * ROWB + chunk * 16) = b;
    }
  };

  floatx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int nsteps = (pend - pbeg + WG_BK - 1) / WG_BK;
  if (nsteps > 0) {
    load(pbeg);
    store(0);
  }
  __syncthreads();
  const int li = lane & 31, lh = lane >> 5;
  // transposed-read addressing (bf16): 16-lane group g16, lane-in-group 4*trq + trp
  const int g16 = lane >> 4, lig = lane & 15;
  const int trq = lig >> 2, trp = lig & 3;
  const int trh = g16 >> 1, trc = 16 * (g16 & 1) + 4 * trp;
  for (int s = 0; s < nsteps; ++s) {
    const int cur = s & 1;
    if (s + 1 < nsteps) load(pbeg + (s + 1) * WG_BK);
    const char* sA = smem + cur * 2 * TILEB;
    const char* sB = sA + TILEB;
    if constexpr (sizeof(T) == 4) {
#pragma unroll 4
      for (int kk = 0; kk < WG_BK / 2; ++kk) {
        const int k = 2 * kk + lh;
        const float* ra = reinterpret_cast<const float*>(sA + k * ROWB);
        const float* rb = reinterpret_cast<const float*>(sB + k * ROWB);
        const float a0 = ra[wm * 64 + li], a1 = ra[wm * 64 + 32 + li];
        const float b0 = rb[wn * 64 + li], b1 = rb[wn * 64 + 32 + li];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < WG_BK / 16; ++ks) {
        bf16x8 fa[2], fb[2];
        const int row = ks * 16 + 8 * trh + trq;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const char* pa = sA + row * ROWB + (wm * 64 + 32 * i + trc) * 2;
          const char* pb = sB + row * ROWB + (wn * 64 + 32 * i + trc) * 2;
          const v4i16 a_lo = lds_tr16(pa), a_hi = lds_tr16(pa + 4 * ROWB);
          const v4i16 b_lo = lds_tr16(pb), b_hi = lds_tr16(pb + 4 * ROWB);
          const v8i16 av = {a_lo[0], a_lo[1], a_lo[2], a_lo[3], a_hi[0], a_hi[1], a_hi[2], a_hi[3]};
          const v8i16 bv = {b_lo[0], b_lo[1], b_lo[2], b_lo[3], b_hi[0], b_hi[1], b_hi[2], b_hi[3]};
          fa[i] = __builtin_bit_cast(bf16x8, av);
          fb[i] = __builtin_bit_cast(bf16x8, bv);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
    }
    if (s + 1 < nsteps) store(cur ^ 1);
    __syncthreads();
  }

  if (p.dW) {  // single pixel split: write torch layout dW[r][ci][kh][kw] directly
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = c0 + wn * 64 + 32 * j + li;
      const int tt = n / p.Cg, cc = n - tt * p.Cg;
      if (n >= p.Ncol || cc >= p.Cg_out) continue;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = r0 + wm * 64 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * lh;
          if (m < p.R) p.dW[((long long)m * p.Cg_out + cc) * 16 + tt] = acc[i][j][e];
        }
    }
    return;
  }
  float* slab = p.ws + (long long)split * p.R * p.Ncol;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = c0 + wn * 64 + 32 * j + li;
      if (n >= p.Ncol) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = r0 + wm * 64 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (m < p.R) slab[(long long)m * p.Ncol + n] = acc[i][j][e];
      }
    }
