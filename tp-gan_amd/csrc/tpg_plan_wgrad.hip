// Weight-gradient planner (tpg_plan.h): kernel family, tile, pixel split and every launch
// argument that needs no data pointer.  Host arithmetic on the descriptor, dtypes and strides only.
#include "tpg_plan.h"
#include "../../include/tpgan.h"

namespace tpg {

// Row-halo weight gradient (tpg_wgrad_rh.hip) for a stride-1 Conv2d: false when the shape is
// not covered (the caller falls back).
static bool plan_wgrad_rh(const PlanCtx& cx, const tpg_conv_desc* d, const tpg_tensor& x, const tpg_tensor& g,
                          const tpg_tensor& dw, WgradPlan* p) {
  if (!half16(d->dtype) || d->stride_h != 1 || d->stride_w != 1) return false;
  const int PH = d->out_h, PW = d->out_w, QH = d->in_h, QW = d->in_w;
  // row mode: one kernel row, 3/5/7 taps, 64-pixel row segments; image mode (algos 10, 11 and
  // the default below 64 pixels of width): all taps of a 2x2 / 3x3 kernel from one halo of
  // (64 / tw) whole rows of width tw
  const bool row_ok = PW % 64 == 0 && (d->kw == 3 || d->kw == 5 || d->kw == 7);
  // algo 13: the dense tap-per-wave tile, one block per kernel row of a 7-wide kernel with all
  // (<= 80) channels of both sides
  const bool dense = d->algo == 13;
  if (dense && (d->kw != 7 || d->out_c > 80 || d->in_c > 80)) return false;
  // algo 14: the dense five-tap tile, one block per kernel row of a 5-wide kernel and (a, b) tile
  const bool dense5 = d->algo == 14;
  if (dense5 && d->kw != 5) return false;
  // image mode k-tile: th = floor(64 / tw) rows of tw = min(PW, 64); the fragment reads reach
  // halo row (63 / tw + kh - 1) * (tw + kw - 1) + tw + kw - 2, inside the 200-row LDS image
  const int tw = std::min(PW, 64);
  const bool img_ok = d->kh == d->kw && (d->kw == 2 || d->kw == 3) && PW % tw == 0 && tw >= 4 &&
                      (63 / tw + d->kh - 1) * (tw + d->kw - 1) + tw + d->kw - 2 < 200;
  // (untuned default only for full 64-pixel k-tiles: 40-wide maps measured slower than wgrad2)
  const bool img = d->algo == 10 || d->algo == 11 || (d->algo == 0 && !row_ok && 64 % tw == 0);
  if (img ? !img_ok : !row_ok) return false;
  if (d->pad_t >= QH || d->pad_l >= QW || !vec_ok(g, d->dtype) || !vec_ok(x, d->dtype)) return false;
  if (g.stride[2] != (int64_t)PW * g.stride[3] || g.stride[0] != (int64_t)PH * g.stride[2]) return false;
  if (x.stride[2] != (int64_t)QW * x.stride[3] || x.stride[0] != (int64_t)QH * x.stride[2]) return false;
  // extents cover the last pixel's whole 16-byte chunks (vec_ok: pixel stride >= ceil8(C))
  const int64_t pb = ((int64_t)(d->n - 1) * g.stride[0] + (int64_t)(PH - 1) * g.stride[2] +
                      (int64_t)(PW - 1) * g.stride[3] + rup(d->out_c, 8)) * 2;
  const int64_t qb = ((int64_t)(d->n - 1) * x.stride[0] + (int64_t)(QH - 1) * x.stride[2] +
                      (int64_t)(QW - 1) * x.stride[3] + rup(d->in_c, 8)) * 2;
  if (pb >= (1ll << 31) || qb >= (1ll << 31)) return false;
  WgradRHArgs& a = p->rh;
  a.dtype = d->dtype;
  a.p_sn = (int)g.stride[0]; a.p_sh = (int)g.stride[2]; a.p_sw = (int)g.stride[3];
  a.PH = PH; a.PW = PW; a.Ca = d->out_c; a.p_bytes = (int)pb;
  a.q_sn = (int)x.stride[0]; a.q_sh = (int)x.stride[2]; a.q_sw = (int)x.stride[3];
  a.QH = QH; a.QW = QW; a.Cb = d->in_c; a.q_bytes = (int)qb;
  a.kh = d->kh; a.kw = d->kw; a.pt = d->pad_t; a.pl = d->pad_l; a.pad_mode = d->pad_mode;
  a.nr = img ? d->kh : 1;
  a.nrg = cdiv(a.kh, a.nr);
  a.tw = img ? tw : 64;
  // tile: fewest padded MACs, the 128 x 64 tile (best operand reuse) on ties
  int bm = 128, bc = 64;
  if (d->algo >= 6 && d->algo <= 14) {
    a.cfg = d->algo - 6;
    wgrad_rh_tile(a.cfg, &bm, &bc);
    if (dense5) {
      // channel tiles padded by at most one MFMA block: ceil(C / 112) tiles of ceil(C / tiles)
      // channels, rounded up to 16 (206 -> 2 x 112, 80 -> 80, 64 -> 64)
      bm = (int)rup(cdiv(a.Ca, cdiv(a.Ca, bm)), 16);
      bc = (int)rup(cdiv(a.Cb, cdiv(a.Cb, bc)), 16);
      a.tm = bm; a.tn = bc;
    }
  } else {
    int64_t best = -1;
    for (int c = img ? 4 : 0; c < (img ? 6 : 4); ++c) {
      int m, b;
      wgrad_rh_tile(c, &m, &b);
      const int64_t cost = rup(a.Ca, m) * rup(a.Cb, b) * (100 + (m == 64 ? 8 : 0) + (b == 32 ? 8 : 0));
      if (best < 0 || cost < best) { best = cost; a.cfg = c; bm = m; bc = b; }
    }
  }
  // taps per block: a whole kernel row, except 7-wide rows on the 128 x 64 / 256 x 32 tiles
  // (7 x BC columns there exceed the VGPR budget: 4 + 4 taps, one of them dead)
  a.nt = img ? d->kw : (d->kw == 7 && (a.cfg == 0 || a.cfg == 6)) ? 4 : d->kw;
  a.nta = cdiv(a.Ca, bm); a.ntb = cdiv(a.Cb, bc);
  a.tiles = a.nta * a.ntb * a.nrg * cdiv(a.kw, a.nt);
  a.nkt = d->n * cdiv(PH, 64 / a.tw) * (PW / a.tw);
  int ks = 1;
  if (d->algo >= 6 && d->ksplit >= 1) {
    ks = d->ksplit;
  } else {
    // pixel splits: whole rounds of resident blocks (one per CU, two for the <= 128-VGPR
    // tiles) against the fp32 atomics every extra split adds (~1.3 TB/s of added bytes)
    const int resident = (img || a.cfg >= 6 ? 256 : (a.cfg == 3 || (a.cfg != 0 && a.nt <= 4)) ? 512 : 256) / cx.share;
    const int taps = a.nr * a.nt;
    const double flops = 2.0 * a.tiles * bm * taps * bc * 64.0 * a.nkt;
    double best = -1;
    for (int k = 1; k <= 64 && k <= a.nkt; ++k) {
      const int64_t blocks = (int64_t)a.tiles * k;
      const double rounds = (double)((blocks + resident - 1) / resident);
      const double t = rounds * flops / blocks / (4.5e12 * 256 / resident) +
                       (k > 1 ? k * (double)a.tiles * bm * taps * bc * 4 / 1.3e12 : 0.0);
      if (best < 0 || t < best) { best = t; ks = k; }
    }
  }
  ks = std::max(1, std::min(ks, a.nkt));
  if (cx.det) ks = 1;  // one block adds each dW element once
  a.kt_per_split = cdiv(a.nkt, ks);
  a.ksplit = cdiv(a.nkt, a.kt_per_split);
  a.w_sa = dw.stride[0]; a.w_sb = dw.stride[1]; a.w_sr = dw.stride[2]; a.w_ss = dw.stride[3];
  // bias MFMAs spread over up to 16 / ksplit tiles: same-address atomics serialise (~50 ns
  // each), so blocks x splits adding into one dbias row must stay few
  a.bshare = cx.det ? 1 : std::max(1, std::min(a.ntb * a.nrg * cdiv(a.kw, a.nt), 16 / a.ksplit));
  a.skip = dense || dense5 ? 0 : 1;  // (the dense tiles have no dead-block skip)
  p->kernel = img ? TPG_WGRAD_IMAGE_HALO : TPG_WGRAD_ROW_HALO;
  p->cfg = a.cfg; p->bm = bm; p->bn = bc; p->tiles = a.tiles;
  return true;
}

// Validates the call and plans it: the row/image-halo kernel where it applies (desc.algo 0 or
// 6..14), else the flat DMA kernel on 16-byte aligned rows, else the generic kernel.
int32_t plan_bwd_filter(const tpg_conv_desc* d, const tpg_tensor& x, const tpg_tensor& g, const tpg_tensor& dw,
                               WgradPlan* p) {
  int32_t rc = check_desc(d);
  if (rc) return rc;
  if ((rc = check_tensor(x, d->dtype, "x")) || (rc = check_tensor(g, d->dtype, "g"))) return rc;
  if (!dw.data || dw.dtype != TPG_F32) return fail(-13, "dw must be fp32");
  const PlanCtx cx = plan_ctx(d);
  memset(p, 0, sizeof(*p));
  WgradArgs& a = p->a;
  p->p_is_x = d->transposed;
  const tpg_tensor& P = d->transposed ? x : g;  // iteration grid operand
  const tpg_tensor& Q = d->transposed ? g : x;  // gathered operand
  const int PH = d->transposed ? d->in_h : d->out_h, PW = d->transposed ? d->in_w : d->out_w;
  const int QH = d->transposed ? d->out_h : d->in_h, QW = d->transposed ? d->out_w : d->in_w;
  const int Ca = d->transposed ? d->in_c : d->out_c, cb = d->transposed ? d->out_c : d->in_c;
  const bool comp = composite(d, &x, &g);
  if (!comp && big_taps(d)) return fail(-4, "%dx%d kernel: only the dense NHWC GEMM form is supported", d->kh, d->kw);
  a.p_sn = P.stride[0]; a.p_sh = P.stride[2]; a.p_sw = P.stride[3];
  a.q_sn = Q.stride[0]; a.q_sh = Q.stride[2]; a.q_sw = Q.stride[3];
  a.Ca = Ca;
  a.vec_p = vec_ok(P, d->dtype);
  a.vec_q = vec_ok(Q, d->dtype);
  if (comp) {
    a.PH = 1; a.PW = 1; a.QH = 1; a.QW = 1;
    a.Cb = d->kh * d->kw * cb;
    a.bcomp = 1; a.comp_kw = d->kw; a.comp_cb = cb;
    a.ntaps = 1; a.dy[0] = 0; a.dx[0] = 0; a.tr[0] = 0; a.ts[0] = 0;
    a.qst_h = 1; a.qst_w = 1;
  } else {
    a.PH = PH; a.PW = PW; a.QH = QH; a.QW = QW; a.Cb = cb;
    a.qst_h = d->stride_h; a.qst_w = d->stride_w;
    a.pad_mode = d->transposed ? 0 : d->pad_mode;
    a.ntaps = d->kh * d->kw;
    for (int r = 0; r < d->kh; ++r)
      for (int s = 0; s < d->kw; ++s) {
        int t = r * d->kw + s;
        a.dy[t] = (int8_t)(r - d->pad_t); a.dx[t] = (int8_t)(s - d->pad_l);
        a.tr[t] = (int8_t)r; a.ts[t] = (int8_t)s;
      }
  }
  a.npix = d->n * a.PH * a.PW;
  a.w_sa = dw.stride[0]; a.w_sb = dw.stride[1]; a.w_sr = dw.stride[2]; a.w_ss = dw.stride[3];
  a.div_pw.init(a.PW);
  a.div_phpw.init(a.PH * a.PW);
  // the bias gradient rides on the halo and flat launches of a Conv2d (its pixel grid is g's)
  p->sums_bias = !d->transposed;
  // kernel-row halo kernel (stride-1 Conv2d, bf16, 64-pixel row segments): algo 6, and the
  // default for untuned calls when it applies
  const bool rh_algo = d->algo >= 6 && d->algo <= 14;
  if ((d->algo == 0 || rh_algo) && !comp && !d->transposed && plan_wgrad_rh(cx, d, x, g, dw, p)) return 0;
  if (rh_algo) return fail(-30, "wgrad: row-halo kernel does not apply to this shape");
  // pipelined DMA kernel when both operands are 16-byte aligned channels-last rows
  if (a.vec_p && a.vec_q) {
    // non-composite: columns flattened over taps (b' = tap * rup(Cb, 8) + b), so channel
    // counts like 75 / 206 waste at most 7 columns per tap instead of a tile remainder
    a.bflat = comp ? 0 : 1;
    a.cbp = (int)rup(a.Cb, 8);
    const int64_t ncols = a.bflat ? (int64_t)a.ntaps * a.cbp : a.Cb;
    const int ngrid = a.bflat ? 1 : a.ntaps;
    // Default tile / pixel-split choice (padded MACs, 64-wide tiles charged 15% for their
    // lower operand reuse; about 2048 blocks).  Callers that autotune pass their choice in
    // the descriptor: algo = tile index + 1 into cand[], ksplit = pixel splits.
    static const int cand[5][2] = {{256, 128}, {128, 128}, {128, 64}, {64, 128}, {64, 64}};
    const int kp = half16(d->dtype) ? 64 : 32;
    const int nkt = cdiv(a.npix, kp);
    int bm = 0, bn = 0, bks = 1;
    {
      int64_t best = -1;
      for (auto& c : cand) {
        const int64_t cost = (int64_t)rup(a.Ca, c[0]) * rup(ncols, c[1]) * ngrid * ((c[0] == 64 || c[1] == 64) ? 115 : 100);
        if (best < 0 || cost < best) { best = cost; bm = c[0]; bn = c[1]; }
      }
      const int tiles = cdiv(a.Ca, bm) * (int)((ncols + bn - 1) / bn) * ngrid;
      bks = std::max(1, cdiv(2048 / cx.share, tiles));
      bks = std::min(bks, std::max(1, a.npix / (kp * 8)));
    }
    if (d->algo >= 1 && d->algo <= 5 && d->ksplit >= 1) {
      bm = cand[d->algo - 1][0]; bn = cand[d->algo - 1][1];
      bks = std::min(d->ksplit, nkt);
    }
    if (cx.det) bks = 1;
    a.pix_per_split = (int)rup(cdiv(a.npix, bks), kp);
    a.ksplit = cdiv(a.npix, a.pix_per_split);
    const int es = esize(d->dtype);
    // byte extent up to the end of the last pixel's last 16-byte chunk (a chunk straddling C
    // must not count as out of range: vec_ok rows are padded to whole chunks)
    auto extent = [&](const tpg_tensor& t, int n, int h, int w, int c) -> int64_t {
      return ((int64_t)(n - 1) * t.stride[0] + (int64_t)(h - 1) * t.stride[2] + (int64_t)(w - 1) * t.stride[3] +
              rup(c, 16 / es)) * es;
    };
    const int64_t pb = extent(P, d->n, a.PH == 1 && comp ? 1 : PH, a.PW == 1 && comp ? 1 : PW, a.Ca);
    const int64_t qb = comp ? extent(Q, d->n, 1, 1, a.Cb) : extent(Q, d->n, QH, QW, cb);
    if (pb < (1ll << 31) && qb < (1ll << 31)) {
      a.p_bytes = (int)pb;
      a.q_bytes = (int)qb;
      // division-free DMA addressing (see tpg_wgrad2.hip)
      a.fastp = !comp && P.stride[2] == (int64_t)PW * P.stride[3] && P.stride[0] == (int64_t)PH * P.stride[2];
      a.fastq = a.bflat && a.qst_h == 1 && a.qst_w == 1 && a.pad_mode == 0 && QH == PH && QW == PW &&
                Q.stride[2] == (int64_t)QW * Q.stride[3] && Q.stride[0] == (int64_t)QH * Q.stride[2] &&
                (int64_t)PH * PW > kp;
      a.dpy = kp / a.PW;
      a.dpx = kp % a.PW;
      a.bshare = cx.det ? 1 : std::max(1, std::min((int)((ncols + bn - 1) / bn) * ngrid, 16 / a.ksplit));
      p->kernel = TPG_WGRAD_FLAT;
      p->cfg = wgrad2_cfg(bm, bn); p->bm = bm; p->bn = bn;
      p->tiles = cdiv(a.Ca, bm) * (int)((ncols + bn - 1) / bn) * ngrid;
      return 0;
    }
  }
  const int cfg = (a.Ca >= 128 && a.Cb >= 128) ? 1 : 0;
  const int bm = wgrad_cfg_bm(cfg), bn = wgrad_cfg_bn(cfg);
  const int tiles = cdiv(a.Ca, bm) * cdiv(a.Cb, bn) * a.ntaps;
  int ks = std::max(1, cdiv(1536, tiles));
  ks = std::min(ks, std::max(1, a.npix / (32 * 16)));
  if (cx.det) ks = 1;
  a.pix_per_split = (int)rup(cdiv(a.npix, ks), 32);
  a.ksplit = cdiv(a.npix, a.pix_per_split);
  p->kernel = TPG_WGRAD_GENERIC;
  p->cfg = cfg; p->bm = bm; p->bn = bn; p->tiles = tiles;
  p->sums_bias = false;  // (the generic kernel has no bias sum)
  return 0;
}

}  // namespace tpg
