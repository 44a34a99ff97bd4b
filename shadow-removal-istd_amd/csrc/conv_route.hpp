// Host-side interface between the conv files: the two functions that decide which kernel a call runs -- conv_route
// (conv_route.cpp) for the forward and input-gradient convs, wgrad_route (wgrad_route.cpp) for the weight gradient; the
// tables are DESIGN.md section 4 -- and every function one .hip file calls in another, declared once: the defining
// file includes this header, so the compiler checks each signature.
#pragma once
#include "common.hpp"

namespace stc {

struct GParams;  // igemm_bf16.hpp

// ---- plans of the two tile kernels (chosen by the file that owns the kernel, carried by the route)
struct FpPlan {  // igemm.hip: the register-staged igemm_kernel
  int BM, BN, ksplit, kchunk, mtiles, ntiles;
};
struct BPlan {  // igemm_bf16.hip: the LDS-DMA tile
  int cfg;      // index into the tile table
  int BM, BN, ksplit, kchunk, mtiles, ntiles;
};
struct Bf16Problem {
  int M, N, K, nphase;
  BPlan pl;
  bool vec_out;
  int64_t ws_bytes;
  int stats_chunks;
  int reduce_rows;
  bool wide;      // split-K reduction by splitk_reduce_wide_kernel (a chunk per row)
  bool inlaunch;  // split-K combined in the launch (GParams::slab / tickets): the tile statistics of one launch
};

// ---- the route
// force_plan {HALO_CFG, shape}: the halo kernel (an error where it is not eligible)
constexpr int HALO_CFG = 100;

struct ConvAsk {  // everything the choice of kernel depends on
  int dtype, kind, B;
  stc_view x, y;
  int Cin, Cout;
  bool prologue;
  int tanh;  // the epilogue's output head, an STC_HEAD_* code; the route reads only whether it is non-zero
  bool out_f32;
  bool stats;               // BatchNorm statistics of the output wanted
  const stc_bnb_fuse* bnb;  // BN-backward sums wanted (bnb_act: the activation backward of a layer without BN instead)
  bool bnb_act;
  int act_n;  // activation epilogue: 1 or 2 activated copies (the second into *act2)
  const stc_view* act2;
  const int32_t* force;  // force_plan
  // STC_PAD_ZEROS, or STC_PAD_REFLECT.  A reflect ask of a Conv2d kind is the layer's forward;
  // one of kind STC_CONVT_S2 / STC_CONV_S1_DGRAD is the layer's input gradient, y the gradient of its input: the
  // padding-free transposed conv over the extended grid into an fp32 frame, then the fold
  int pad;
};

enum ConvKernel { CONV_NONE, FP_TILE, SMALLN, NARROW_TILED, BF16_NARROW, STEM, STEM_S1D, HALO, BF16_TILE };

struct ConvRoute {
  ConvKernel kernel;  // CONV_NONE: no kernel takes the activation form asked for (stc_conv_*_act_ok = 0)
  bool fused;         // the kernel itself computes the statistics / BN-backward sums / activation asked for
  int64_t ws_bytes;
  int chunks;        // statistics / BN-backward partials: of the kernel when fused, else of the pass that follows it
  int32_t plan[5];   // {BM, BN, ksplit, narrow, tile config} as stc_conv_fwd_query reports it
  // what the launcher needs and does not derive again
  int GH, GW;                   // the GEMM grid
  bool vec_out;                 // GParams::vec_out
  int halo_shape;               // HALO: the forced block shape (0: automatic)
  const int32_t* narrow_force;  // BF16_NARROW: the forced tile, or NULL
  FpPlan fp;                    // FP_TILE
  Bf16Problem bf;               // BF16_TILE
  // a reflect input gradient: the fp32 frame [B][FH][FW][Cout] at the head of the workspace (frame_bytes of
  // ws_bytes; 0 for every other ask), the split-K slabs behind it
  int FH, FW;
  int64_t frame_bytes;
};

ConvRoute conv_route(const ConvAsk& a);

struct ConvOps {  // what a launch takes besides the ask: operands, results, scratch
  const void* w;
  const float* bias;
  const float *pro_scale, *pro_shift;
  int pro_act;
  float pro_slope;
  float* stats;
  int stats_chunks;  // of stats or part2
  float* part2;
  float act_s1, act_s2;
  void* ws;
  int64_t ws_bytes;
  hipStream_t st;
};

// 16-byte vector access to every pixel of a bf16 NHWC view
static inline bool vec16_view(const stc_view& v) {
  return v.cs == 1 && v.co % 8 == 0 && v.ps % 8 == 0 && v.rs % 8 == 0 && v.bs % 8 == 0 && ((uintptr_t)v.p & 15) == 0;
}

// ---- igemm.hip
bool use_smalln(int dtype, int N, int K);
bool narrow_tiled_eligible(int dtype, int kind, int Cin);
FpPlan fp_tile_plan(int dtype, int M, int N, int K, int nphase);

// ---- igemm_bf16.hip
bool vec_out_ok(int B, const stc_view& y, int Cout, int out_f32);
bool bf16_conv_eligible(int kind, int B, const stc_view& x, int Cin, int Cout);
Bf16Problem bf16_problem(int M, int N, int K, int nphase, const int32_t* force, bool vec_out);  // reads the in-launch split-K switch
int bf16_igemm_launch(GParams& p, const Bf16Problem& pr, void* ws, int64_t ws_bytes, float* stats, int stats_chunks,
                      hipStream_t st);
// launches r.kernel, one of STEM, STEM_S1D, HALO, BF16_TILE
int bf16_conv_fwd(const ConvAsk& a, const ConvRoute& r, const ConvOps& o);

// ---- halo_bf16.hip
bool halo_geometry_ok(int kind, int B, int GH, int GW, int Cin, int Cout);
bool halo_auto(int kind, int B, int GH, int GW, int Cin, int Cout);
bool halo_eligible(int kind, int B, const stc_view& x, int Cin, int Cout, const stc_view& y);
int halo_chunks(int kind, int B, int GH, int GW);
int halo_plan_bn(int kind, int B, int GH, int GW, int Cout, int shape);
int halo_launch(GParams& p, hipStream_t st, int shape);

// ---- stem_bf16.hip: the Cin = 8 first layers, the logits layer's input gradient
bool stem_eligible(int kind, int B, const stc_view& x, int Cin, int Cout, const stc_view& y, bool bnb);
bool stem_s1d_eligible(int kind, int B, const stc_view& dy, int Cin, int Cout, const stc_view& y);
int stem_bnb_chunks(int kind, int B, int Hg, int Wg, int Cin, int Cout);
int stem_launch(GParams& p, hipStream_t st);
int stem_s1d_launch(GParams& p, hipStream_t st);

// ---- narrow_bf16.hip
bool bf16_narrow_eligible(int kind, int Cin, int Cout);
int64_t bf16_narrow_workspace(int kind, int B, int GH, int GW, int Cin, int Cout);
int bf16_narrow_fwd(int kind, int B, stc_view x, int Cin, const void* w_packed, int Cout, stc_view y,
                    const float* bias, int epi_tanh, int out_f32, void* ws, int64_t ws_bytes, hipStream_t st,
                    const int32_t* force);

// ---- the weight gradient's route (wgrad_route, wgrad_route.cpp; the table is DESIGN.md section 4)
struct WgPlan {  // wgrad.hip: the register-staged wgrad_kernel / wgrad_reflect_kernel
  int BM, BN, mtiles, ntiles, nsplit, pchunk;
};
struct WbPlan {  // wgrad_bf16.hip: the LDS-DMA tiles and the halo tile
  int cfg, BM, BN, mtiles, ntiles, nsplit, pchunk;
  bool slab;    // partial sums go to fp32 slabs + the ordered reduce (always when nsplit > 1)
  bool cmajor;  // channel-group-major columns (WbParams::cmajor): one split whose tiles store torch layout directly
  bool s1v;     // planned over the stride-1 halo tile's virtual grid (GH + 1) x (GW + 1)
};

struct WgradAsk {  // everything the choice of kernel depends on
  int dtype, B, stride;
  stc_view D, G;
  int R, Cg, Cg_out;
  int rows;          // real channels of D when the rest is padding; 0: not asked / the rows kernels off
  bool rows_direct;  // stc_conv_wgrad_rows called directly: its own checks decide, not the automatic LDS budget
  bool prologue;     // any of d / g scale, shift, activation
  int pad;           // STC_PAD_ZEROS / STC_PAD_REFLECT
  const int32_t* force;  // force_plan {tile config, pixel splits}
};

enum WgradKernel { WG_NONE, WG_FP_TILE, WG_BF16_TILE, WG_BF16_LD, WG_HALO, WG_ROWS, WG_ROWS_MFMA };
enum WgradReduce { WR_NONE, WR_PLAIN, WR_V4, WR_MANY };

struct WgradRoute {
  WgradKernel kernel;  // WG_NONE: no pixels (B * D.H * D.W == 0), nothing to launch
  WgradReduce reduce;  // WR_NONE: the kernel writes dW itself
  int64_t ws_bytes;
  int32_t plan[5];  // {tile config (-1: none), BM, BN, slabs, slab} as stc_conv_wgrad_query reports it
  // what the launchers need and do not derive again
  int slabs;  // fp32 slabs the reduce sums (0: none)
  WgPlan fp;  // WG_FP_TILE
  WbPlan wb;  // WG_BF16_TILE, WG_BF16_LD, WG_HALO
  int pmode, lg_gw, lg_ghw;  // WbParams' pixel mapping
  int GH, GW;                // the reduction grid: D's, or the stride-1 halo tile's virtual grid
  int halo_tc;               // WG_HALO: grid columns per tile row (8 .. 64)
  bool halo_s1;              // WG_HALO: the stride-1 form
  int rows_parts;            // WG_ROWS / WG_ROWS_MFMA: slabs per image
  size_t lds;                // dynamic LDS bytes of the launch
  char name[96];             // the kernel as a profiler prints it (the timer label)
};

WgradRoute wgrad_route(const WgradAsk& a);

// bytes of nsplit fp32 slabs [R][16 Cg]
static inline int64_t wgrad_slab_bytes(int nsplit, int R, int Cg) { return (int64_t)nsplit * R * 16LL * Cg * 4; }

// a dense NHWC view of a shape-only query: no pointer, batch stride 0
static inline stc_view dense_view(int H, int W, int C) {
  stc_view v{};
  v.H = H; v.W = W; v.rs = (int64_t)W * C; v.ps = C; v.cs = 1;
  return v;
}

// ---- wgrad.hip
WgPlan wg_plan(int P, int R, int Cg);
WgradReduce wgrad_reduce_kind(int nsplit, int R, int Cg, int Cg_out);
void wgrad_reduce_launch(WgradReduce kind, const float* ws, int nsplit, int R, int Cg, int Cg_out, float* dW,
                         hipStream_t st);
// which rows kernel takes the ask by the kernels' own conditions (WG_NONE: neither); fills rows_parts, lds
WgradKernel wgrad_rows_kind(const WgradAsk& a, WgradRoute& r);

// ---- wgrad_bf16.hip
bool wgrad_bf16_eligible(int B, const stc_view& D, int R, const stc_view& G, int Cg);
// g_on_grid: G is exactly the doubled grid (stride 2) / the grid + 1 (stride 1), which the halo tile needs
WbPlan wb_plan(int B, int GH, int GW, int stride, bool g_on_grid, int R, int Cg, const int32_t* force);
// the launch of plan r.wb on the D grid GH x GW: kernel, pixel mapping, reduction grid, LDS bytes, name
void wb_launch_shape(int GH, int GW, WgradRoute& r);
// launches r.kernel, one of WG_BF16_TILE, WG_BF16_LD, WG_HALO
int wgrad_bf16(const WgradAsk& a, const WgradRoute& r, float* dW, void* workspace, int64_t workspace_bytes,
               hipStream_t st);

}  // namespace stc
