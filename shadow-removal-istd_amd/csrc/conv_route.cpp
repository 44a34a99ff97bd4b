// Which kernel a conv call runs, and what follows from that (workspace, chunk count, plan): decided here and nowhere
// else.  The queries and the launchers of igemm.hip all ask conv_route; the eligibility predicates stay with their
// kernels and are called from here only.  DESIGN.md section 4 has the table.
#include "conv_route.hpp"

namespace stc {

ConvRoute conv_route(const ConvAsk& a) {
  ConvRoute r{};
  const Geometry g = geometry(a.kind);
  const int taps = g.taps_lg_tw == 2 ? 16 : 4;
  const bool convt = a.kind == STC_CONVT_S2;
  const int kind = a.kind, B = a.B, Cin = a.Cin, Cout = a.Cout;
  const int GH = convt ? a.x.H : a.y.H, GW = convt ? a.x.W : a.y.W;  // the GEMM grid
  const int M = B * GH * GW, K = taps * Cin;
  r.GH = GH;
  r.GW = GW;
  if (a.pad == STC_PAD_REFLECT) {
    // Reflect padding: only the two gather kernels of igemm.hip implement it -- the register-staged tile and the
    // wave-per-pixel narrow-N kernel -- and nothing is fused: statistics, BN-backward sums and activations come
    // from passes over the stored output (for the input gradient they would be formed before the fold).
    if (a.prologue || a.bnb || a.act_n) return r;  // CONV_NONE: no such form
    const bool dgrad = convt || kind == STC_CONV_S1_DGRAD;
    int gh = GH, gw = GW;
    if (dgrad) {  // the frame conv's grid: every index -1 .. H of the input gradient's extent (y), per phase for s2
      gh = convt ? (a.y.H + 3) / 2 : a.y.H + 2;
      gw = convt ? (a.y.W + 3) / 2 : a.y.W + 2;
      r.FH = convt ? 2 * gh : gh;
      r.FW = convt ? 2 * gw : gw;
      r.frame_bytes = (int64_t)B * r.FH * r.FW * Cout * 4;
    }
    r.GH = gh;
    r.GW = gw;
    const int m = B * gh * gw;
    const long long P = (long long)m * (g.nphase == 4 ? 4 : 1);
    r.chunks = stc_chan_stats_chunks(1, 1, (int)std::min<long long>(P, 1 << 30));
    r.plan[2] = 1;
    r.plan[4] = -1;
    if (use_smalln(a.dtype, Cout, K)) {
      r.kernel = SMALLN;
      r.plan[0] = 1; r.plan[1] = Cout; r.plan[3] = 1;
      r.ws_bytes = r.frame_bytes;
      return r;
    }
    r.kernel = FP_TILE;
    r.fp = fp_tile_plan(a.dtype, m, Cout, K, g.nphase);
    r.ws_bytes = r.frame_bytes + (r.fp.ksplit <= 1 ? 0 : (int64_t)g.nphase * r.fp.ksplit * (int64_t)m * Cout * 4);
    r.plan[0] = r.fp.BM; r.plan[1] = r.fp.BN; r.plan[2] = r.fp.ksplit;
    return r;
  }
  const bool plain = a.dtype == STC_BF16 && !a.prologue;  // what the bf16-only kernels take
  auto smalln_at = [&](int k) { return use_smalln(a.dtype, Cout, k); };
  auto vec_out = [&](const stc_view& v, bool f32) { return vec_out_ok(B, v, Cout, f32) && Cout % 8 == 0; };
  const bool smalln = smalln_at(K);
  const bool bf16_family = plain && !a.tanh && !smalln && bf16_conv_eligible(kind, B, a.x, Cin, Cout);
  r.vec_out = bf16_family && vec_out(a.y, a.out_f32);
  // (the BN backward is routed on the output's alignment alone: one of 2^31 elements or more keeps the fused
  // kernel's chunk count and is refused by its launch, not rerouted)
  const bool vec = a.bnb && !a.bnb_act ? bf16_family && vec16_view(a.y) : r.vec_out;

  // The fused epilogues live in the bf16 kernels and store 16-byte NHWC pixels.  Without them the BN backward runs
  // unfused -- the route of the plain conv, then stc_bn_bwd_reduce; the activation forms have no fallback here.
  if ((a.bnb || a.act_n) && !vec) {
    if (a.bnb_act || a.act_n) return r;
    ConvAsk plain_ask = a;
    plain_ask.bnb = nullptr;
    r = conv_route(plain_ask);
    r.fused = false;
    r.chunks = stc_chan_stats_chunks(B, a.bnb->x.H, a.bnb->x.W);
    return r;
  }
  r.plan[2] = 1;
  r.plan[4] = -1;

  if (!bf16_family) {
    // statistics come from stc_chan_stats over the stored output
    const long long P = (long long)B * GH * GW * (g.nphase == 4 ? 4 : 1);
    r.chunks = stc_chan_stats_chunks(1, 1, (int)std::min<long long>(P, 1 << 30));
    if (!smalln) {
      r.kernel = FP_TILE;
      r.fp = fp_tile_plan(a.dtype, M, Cout, K, g.nphase);
      r.ws_bytes = r.fp.ksplit <= 1 ? 0 : (int64_t)g.nphase * r.fp.ksplit * (int64_t)M * Cout * 4;
      r.plan[0] = r.fp.BM; r.plan[1] = r.fp.BN; r.plan[2] = r.fp.ksplit;
      return r;
    }
    r.plan[0] = 1; r.plan[1] = Cout; r.plan[3] = 1;
    if (plain && bf16_narrow_eligible(kind, Cin, Cout)) {
      r.kernel = BF16_NARROW;
      r.ws_bytes = bf16_narrow_workspace(kind, B, GH, GW, Cin, Cout);
      // tuning hook: force_plan = {tile rows, 16-column blocks}
      if (a.force && !a.stats && smalln_at(16 * Cin)) r.narrow_force = a.force;
    } else {
      r.kernel = narrow_tiled_eligible(a.dtype, kind, Cin) ? NARROW_TILED : SMALLN;
    }
    return r;
  }

  r.fused = true;
  const bool force_halo = a.force && a.force[0] == HALO_CFG;
  const bool halo = (force_halo ? halo_geometry_ok(kind, B, GH, GW, Cin, Cout)
                                : (!a.force || a.force[0] == -1) && halo_auto(kind, B, GH, GW, Cin, Cout)) &&
                    vec && halo_eligible(kind, B, a.x, Cin, Cout, a.y);
  const bool streaming = vec && !a.force && !a.stats;  // the stem kernels: no plan to force, no statistics
  const int stem_chunks = a.bnb ? stem_bnb_chunks(kind, B, GH, GW, Cin, Cout) : 0;
  auto same_extent = [&](const stc_view& v) { return v.H == a.y.H && v.W == a.y.W; };

  if (a.bnb_act) {  // in the halo kernels' BN-backward epilogue only, every view 16-byte NHWC bf16 of one extent
    auto vec_side = [&](const stc_view& v) { return same_extent(v) && vec16_view(v) && (long long)B * v.bs < (1ll << 31); };
    const stc_view& x = a.bnb->x;
    const stc_view& go = a.bnb->g_other;
    if (a.force || a.bnb->C != Cout || a.bnb->ch_off != 0 || !halo || !x.p || !vec_side(x) || (go.p && !vec_side(go)))
      return r;
  } else if (a.act_n && a.act2 && a.act2->p && !(vec_out(*a.act2, false) && same_extent(*a.act2))) {
    return r;
  } else if (streaming && a.bnb && !a.bnb->g_other.p && stem_s1d_eligible(kind, B, a.x, Cin, Cout, a.y)) {
    r.kernel = STEM_S1D;
    r.chunks = stem_chunks;
    return r;
  } else if (streaming && (a.act_n || a.bnb) && stem_eligible(kind, B, a.x, Cin, Cout, a.y, a.bnb != nullptr)) {
    r.kernel = STEM;
    r.chunks = stem_chunks;
    return r;
  }
  if (halo && !a.act_n) {
    r.kernel = HALO;
    r.halo_shape = force_halo ? a.force[1] : 0;
    r.chunks = halo_chunks(kind, B, GH, GW);
    r.plan[0] = 256; r.plan[1] = halo_plan_bn(kind, B, GH, GW, Cout, r.halo_shape); r.plan[4] = HALO_CFG;
    return r;
  }
  // (a forced halo plan the shape / views do not allow: bf16_conv_fwd refuses it; the queries answer for the
  // automatic tile)
  r.kernel = BF16_TILE;
  r.bf = bf16_problem(M, Cout, K, g.nphase, force_halo ? nullptr : a.force, vec);
  r.ws_bytes = r.bf.ws_bytes;
  r.chunks = r.bf.stats_chunks;
  r.plan[0] = r.bf.pl.BM; r.plan[1] = r.bf.pl.BN; r.plan[2] = r.bf.pl.ksplit; r.plan[4] = r.bf.pl.cfg;
  return r;
}

}  // namespace stc
