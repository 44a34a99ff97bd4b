// Which kernel a weight-gradient call runs, with what plan, into how much workspace, summed by which reduce: decided
// here and nowhere else.  The queries and launchers of wgrad.hip / wgrad_bf16.hip and the Python wrapper all ask
// wgrad_route; the plan functions stay with their kernels and are called from here only.  DESIGN.md section 4 has the
// table.
#include "conv_route.hpp"

namespace stc {

// The automatic choice of the rows kernels keeps the D plane (2-wide zero border) and the 16 pixel planes' partials of
// the VALU kernel within this many floats of LDS per real row, whichever of the two kernels runs
constexpr long long ROWS_AUTO_FLOATS = 40000, ROWS_PART_FLOATS = 16384;

WgradRoute wgrad_route(const WgradAsk& a) {
  WgradRoute r{};
  const stc_view &D = a.D, &G = a.G;
  r.GH = D.H;
  r.GW = D.W;
  r.plan[0] = -1;
  const long long P = (long long)a.B * D.H * D.W;
  if (P <= 0) return r;  // WG_NONE

  // 1-2 real rows of a stride-1 layer (the PatchGAN logits): each input pixel read once
  if (a.rows > 0 && a.stride == 1 && !a.prologue && !a.force && a.pad == STC_PAD_ZEROS) {
    const WgradKernel k = wgrad_rows_kind(a, r);
    const bool budget = ((long long)(D.H + 4) * (D.W + 4) + ROWS_PART_FLOATS) * a.rows <= ROWS_AUTO_FLOATS;
    if (k != WG_NONE && (a.rows_direct || budget)) {
      r.kernel = k;
      r.slabs = a.B * r.rows_parts;
      r.ws_bytes = wgrad_slab_bytes(a.B * 4, a.rows, a.Cg);  // a slab per (image, pixel split) of the VALU kernel
      r.reduce = wgrad_reduce_kind(r.slabs, a.rows, a.Cg, a.Cg_out);
      r.plan[3] = r.slabs; r.plan[4] = 1;
      snprintf(r.name, sizeof r.name, "%s", k == WG_ROWS_MFMA ? "wgrad_rows_mfma_kernel" : "wgrad_rows_kernel");
      return r;
    }
    r.rows_parts = 0;
  }

  // bf16 without prologues and without reflect: the LDS-DMA family; everything else the register-staged tile
  if (a.pad == STC_PAD_ZEROS && a.dtype == STC_BF16 && !a.prologue && wgrad_bf16_eligible(a.B, D, a.R, G, a.Cg)) {
    // (the stride-2 halo tile needs G on exactly the doubled grid, the stride-1 one on the grid + 1)
    const bool on_grid = a.stride == 2 ? G.H == 2 * D.H && G.W == 2 * D.W : G.H == D.H + 1 && G.W == D.W + 1;
    r.wb = wb_plan(a.B, D.H, D.W, a.stride == 2 ? 2 : 1, on_grid, a.R, a.Cg, a.force);
    wb_launch_shape(D.H, D.W, r);
    r.slabs = r.wb.slab ? r.wb.nsplit : 0;
    r.plan[0] = r.wb.cfg; r.plan[1] = r.wb.BM; r.plan[2] = r.wb.BN; r.plan[3] = r.wb.nsplit; r.plan[4] = r.wb.slab;
  } else {
    r.kernel = WG_FP_TILE;
    r.fp = wg_plan((int)P, a.R, a.Cg);
    r.lds = 0;
    r.slabs = r.fp.nsplit > 1 ? r.fp.nsplit : 0;  // (one split: straight into dW)
    r.plan[1] = r.fp.BM; r.plan[2] = r.fp.BN; r.plan[3] = r.fp.nsplit; r.plan[4] = r.fp.nsplit > 1;
    snprintf(r.name, sizeof r.name, "%s", a.pad == STC_PAD_ZEROS ? "wgrad_kernel" : "wgrad_reflect_kernel");
  }
  r.ws_bytes = r.slabs ? wgrad_slab_bytes(r.slabs, a.R, a.Cg) : 0;
  r.reduce = r.slabs ? wgrad_reduce_kind(r.slabs, a.R, a.Cg, a.Cg_out) : WR_NONE;
  return r;
}

}  // namespace stc
