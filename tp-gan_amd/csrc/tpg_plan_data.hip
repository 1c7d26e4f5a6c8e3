// Forward / input-gradient planner (tpg_plan.h): turns a tpg_conv_desc into implicit-GEMM
// problems (tpg_igemm.hip), routed to the halo or pointwise kernel where they apply.
//
//  op          Conv2d                                  ConvTranspose2d
//  forward     direct form: rows = output pixels,      sub-pixel form: one launch per output
//              A = x gathered at oy*s + r - pad        parity class, taps that reach it
//  bwd_data    sub-pixel form over the input grid,     direct form over the input grid,
//              A = g                                   A = g gathered at iy*s + r - pad
//  bwd_filter  P = g (output grid), Q = x gathered     P = x (input grid), Q = g gathered
//
// A full-kernel conv (Linear fc1 as a 8x8 conv on an 8x8 map) and a transposed conv of a
// 1x1 map (deconv_8) become plain GEMMs over flattened (y, x, c) channels when the
// tensors are dense NHWC ("composite" channels).
#include "tpg_plan.h"
#include "../../include/tpgan.h"
#include <stdlib.h>

namespace tpg {

PlanCtx plan_ctx(const tpg_conv_desc* d) {
  return {(d->flags & TPG_FLAG_CONCURRENT) ? 4 : 1, d->data_ksplit > 0 ? d->data_ksplit : 0,
          (d->data_algo == 1 || d->data_algo == 2) ? d->data_algo : 0, deterministic() != 0};
}

static int choose_cfg(int nout) {
  if (nout <= 16) return 0;
  if (nout <= 32) return 1;
  if (nout <= 64) return 2;
  if (nout <= 96) return 3;
  if (nout <= 128) return 4;
  if (nout > 192 && nout <= 224) return 5;
  return 4;
}

// fill unit / tile / split-K bookkeeping once geometry, C, Nout and taps are known
static void finish(Prob& P, const PlanCtx& cx, int dtype, int M) {
  IgemmArgs& a = P.a;
  const int upk = half16(dtype) ? 4 : 2;
  a.upt = cdiv(std::max(a.C, 1), 16);
  a.nunits = a.ntaps > 0 ? (int)rup((int64_t)a.ntaps * a.upt, upk) : 0;
  a.M = M;
  P.cfg = choose_cfg(a.Nout);
  const int bn = igemm_cfg_bn(P.cfg), bm = igemm_cfg_bm(P.cfg);
  const int npad = (int)rup(a.Nout, bn);
  P.wp_bytes = (size_t)rup((int64_t)npad * a.nunits * 16 * esize(dtype), 256);
  const int nkt = a.nunits / upk;
  const int blocks = cdiv(M, bm) * (npad / bn);
  a.ksplit = 1;
  a.kt_per_split = std::max(nkt, 1);
  if (!cx.det && (cx.ks > 0 || (blocks < 480 / cx.share && nkt >= 8))) {
    int ks = cx.ks > 0 ? std::min(cx.ks, std::max(nkt, 1))  // (an autotuner's pick)
                      : std::min(cdiv(960 / cx.share, blocks), nkt / 4);
    if (ks > 1) {
      a.kt_per_split = cdiv(nkt, ks);
      a.ksplit = cdiv(nkt, a.kt_per_split);
    }
  }
  P.sk_bytes = a.ksplit > 1 ? (size_t)rup((int64_t)M * a.Nout * 4, 256) : 0;
  a.div_jw.init(a.JW);
  a.div_jhjw.init(a.JH * a.JW);
  PackArgs& k = P.pk;
  k.Npad = npad;
  k.Nreal = a.Nout;
  k.nunits = a.nunits;
  k.upt = a.upt;
  k.ntaps = a.ntaps;
  k.Creal = a.C;
  k.dtype = dtype;
}

// direct form: output grid OH x OW (one class), A pixel = o*s + (r - pad)
static Prob direct_prob(int N, int OH, int OW, int kh, int kw, int sh, int sw, int pt, int pl) {
  Prob P;
  IgemmArgs& a = P.a;
  a.JH = OH; a.JW = OW; a.oy0 = 0; a.ox0 = 0; a.osy = 1; a.osx = 1; a.ist_h = sh; a.ist_w = sw;
  a.ntaps = kh * kw;
  for (int r = 0; r < kh; ++r)
    for (int s = 0; s < kw; ++s) {
      int t = r * kw + s;
      a.dy[t] = (int8_t)(r - pt); a.dx[t] = (int8_t)(s - pl);
      P.pk.tr[t] = (int8_t)r; P.pk.ts[t] = (int8_t)s;
    }
  (void)N;
  return P;
}

// sub-pixel form: out grid OH x OW, class (py, px); A pixel = j + (p + pad - r)/s
static std::vector<Prob> subpixel_probs(int OH, int OW, int kh, int kw, int sh, int sw, int pt, int pl) {
  std::vector<Prob> v;
  for (int py = 0; py < sh; ++py)
    for (int px = 0; px < sw; ++px) {
      if (py >= OH || px >= OW) continue;
      Prob P;
      IgemmArgs& a = P.a;
      a.JH = cdiv(OH - py, sh); a.JW = cdiv(OW - px, sw);
      a.oy0 = py; a.ox0 = px; a.osy = sh; a.osx = sw; a.ist_h = 1; a.ist_w = 1;
      int t = 0;
      for (int r = 0; r < kh; ++r) {
        if (pmod(py + pt - r, sh) != 0) continue;
        for (int s = 0; s < kw; ++s) {
          if (pmod(px + pl - s, sw) != 0) continue;
          a.dy[t] = (int8_t)((py + pt - r) / sh);
          a.dx[t] = (int8_t)((px + pl - s) / sw);
          P.pk.tr[t] = (int8_t)r; P.pk.ts[t] = (int8_t)s;
          ++t;
        }
      }
      a.ntaps = t;
      v.push_back(P);
    }
  return v;
}

// stride 2 on maps of <= 64 x 64 outputs (64x64: conv2
// s2 dgrad 0.096 -> 0.039 ms, step -0.3 ms); stride 4 likewise (deconv_32, D_and_G_model.py:220:
// sixteen parity classes, four of them without a tap: 0.138 -> 0.023 ms).  (Thin layers on
// larger maps stay in class form: deconv_128, 16 -> 8 channels at 128x128, measured 54 -> 63 us
// in the zero-insertion form.)
static bool use_dilated(int OH, int OW, int kh, int kw, int sh, int sw, int pad_mode) {
  return sh == sw && (sh == 2 || sh == 4) && pad_mode == TPG_PAD_ZERO && kh <= 5 && kw <= 5 &&
         OH * OW <= 64 * 64;
}

// zero-insertion form of the same problem (stride-2, small maps): ONE unit-stride problem
// over the whole OH x OW grid reading A dilated by s (A pixel (y + pt - r) / s when
// divisible, else zero), all taps; 4x the MACs of the class form, one launch instead of
// four on maps where each class launch is mostly fixed cost
static Prob dilated_prob(int OH, int OW, int kh, int kw, int s, int pt, int pl) {
  Prob P;
  IgemmArgs& a = P.a;
  a.JH = OH; a.JW = OW; a.oy0 = 0; a.ox0 = 0; a.osy = 1; a.osx = 1; a.ist_h = 1; a.ist_w = 1;
  a.dil = s;
  int t = 0;
  for (int r = 0; r < kh; ++r)
    for (int c = 0; c < kw; ++c) {
      a.dy[t] = (int8_t)(pt - r);
      a.dx[t] = (int8_t)(pl - c);
      P.pk.tr[t] = (int8_t)r; P.pk.ts[t] = (int8_t)c;
      ++t;
    }
  a.ntaps = t;
  return P;
}

static bool dense_nhwc(const tpg_tensor& t, int C, int H, int W) {
  return t.stride[1] == 1 && t.stride[3] == C && t.stride[2] == (int64_t)W * C;
}

bool vec_ok(const tpg_tensor& t, int dtype) {
  const int es = esize(dtype);
  if (t.stride[1] != 1) return false;
  if (((uintptr_t)t.data) % 16) return false;
  for (int i : {0, 2, 3})
    if ((t.stride[i] * es) % 16) return false;
  return true;
}

// geometry of a full-kernel conv (kernel = input map, 1x1 output) or a transposed conv of a
// 1x1 map (output = kernel), no padding: the composite-channel GEMM forms
static bool gemm_form(const tpg_conv_desc* d) {
  if (d->pad_t || d->pad_b || d->pad_l || d->pad_r || d->pad_mode) return false;
  if (!d->transposed) return d->in_h == d->kh && d->in_w == d->kw && d->out_h == 1 && d->out_w == 1;
  return d->in_h == 1 && d->in_w == 1 && d->out_h == d->kh && d->out_w == d->kw;
}
bool big_taps(const tpg_conv_desc* d) { return d->kh * d->kw > TPG_MAX_TAPS; }

int32_t check_desc(const tpg_conv_desc* d) {
  if (!d) return fail(-1, "null descriptor");
  if (d->n <= 0 || d->in_c <= 0 || d->out_c <= 0 || d->kh <= 0 || d->kw <= 0) return fail(-2, "bad sizes");
  if (d->stride_h <= 0 || d->stride_w <= 0) return fail(-2, "bad stride");
  // empty maps, and (Conv2d) a kernel larger than the padded input, which C's truncating
  // division would otherwise turn into a 0- or 1-pixel output (torch rejects both)
  if (d->in_h <= 0 || d->in_w <= 0 || d->out_h <= 0 || d->out_w <= 0) return fail(-2, "empty spatial map");
  if (!d->transposed && (d->in_h + d->pad_t + d->pad_b < d->kh || d->in_w + d->pad_l + d->pad_r < d->kw))
    return fail(-6, "kernel %dx%d larger than the padded input", d->kh, d->kw);
  if (d->dtype != TPG_F32 && d->dtype != TPG_BF16 && d->dtype != TPG_F16) return fail(-3, "bad dtype %d", d->dtype);
  // more taps than the tap tables hold: only the full-kernel GEMM forms (fc1 / deconv_8 at
  // 256x256: 16x16 kernels on a 16x16 map or from a 1x1 map), which need no tap table
  if (d->kh * d->kw > TPG_MAX_TAPS && !gemm_form(d))
    return fail(-4, "kernel %dx%d has more than %d taps", d->kh, d->kw, TPG_MAX_TAPS);
  if (d->transposed) {
    if (d->pad_mode != TPG_PAD_ZERO) return fail(-5, "reflect padding is only defined for Conv2d");
    int nh = (d->in_h - 1) * d->stride_h - d->pad_t - d->pad_b + d->kh;
    int nw = (d->in_w - 1) * d->stride_w - d->pad_l - d->pad_r + d->kw;
    if (d->out_h < nh || d->out_w < nw || d->out_h >= nh + d->stride_h || d->out_w >= nw + d->stride_w)
      return fail(-6, "ConvTranspose2d output %dx%d inconsistent with geometry (natural %dx%d)", d->out_h, d->out_w, nh, nw);
  } else {
    int oh = (d->in_h + d->pad_t + d->pad_b - d->kh) / d->stride_h + 1;
    int ow = (d->in_w + d->pad_l + d->pad_r - d->kw) / d->stride_w + 1;
    if (oh != d->out_h || ow != d->out_w) return fail(-6, "Conv2d output %dx%d != %dx%d", d->out_h, d->out_w, oh, ow);
    if (d->pad_mode == TPG_PAD_REFLECT &&
        (d->pad_t >= d->in_h || d->pad_b >= d->in_h || d->pad_l >= d->in_w || d->pad_r >= d->in_w))
      return fail(-7, "reflection padding must be smaller than the input");
  }
  if (std::max(std::abs(d->pad_t), std::abs(d->pad_l)) > 100 || d->kh > 64 || d->kw > 64) return fail(-8, "geometry out of range");
  return 0;
}

int32_t check_tensor(const tpg_tensor& t, int dtype, const char* name) {
  if (!t.data) return fail(-10, "%s is NULL", name);
  if (t.dtype != dtype) return fail(-11, "%s dtype %d != %d", name, t.dtype, dtype);
  if (t.stride[1] != 1) return fail(-12, "%s must be channels-last (channel stride 1), got %lld", name,
                                    (long long)t.stride[1]);
  return 0;
}

// Route a unit-stride (sub-)grid problem to the halo kernel.  Tile choice: a TH x TW tile
// of one image (large maps) or IMG whole images per 256-row block (small maps), minimising
// computed rows x taps plus staged halo pixels; then a split over k-steps when the grid
// has too few blocks to fill the chip (fp32 partial slices, summed by the epilogue).
static void maybe_halo(Prob& P, const PlanCtx& cx, int dtype, int N) {
  IgemmArgs& a = P.a;
  // unit-stride grids, and stride 2 in both directions (halo (2·th + k − 2) x (2·tw + k − 2))
  const int S = a.ist_h;
  if (a.ntaps < 1 || a.C < 1 || a.ist_h != a.ist_w || (S != 1 && S != 2)) return;
  int dymin = 127, dymax = -128, dxmin = 127, dxmax = -128;
  for (int t = 0; t < a.ntaps; ++t) {
    dymin = std::min<int>(dymin, a.dy[t]); dymax = std::max<int>(dymax, a.dy[t]);
    dxmin = std::min<int>(dxmin, a.dx[t]); dxmax = std::max<int>(dxmax, a.dx[t]);
  }
  const int sy = dymax - dymin + 1, sx = dxmax - dxmin + 1;
  if (sy > 7 || sx > 7) return;
  const int JH = a.JH, JW = a.JW;
  // output channels per block first: the 512-row tile (halo up to 1024 pixels) serves the
  // thin layers (BN 64 / 80) of the large maps, where 256 rows run only 8-10 MFMAs per wave
  // between tap barriers; it needs >= 512 blocks (two rounds of the chip) without a k split
  int bn;
  if (a.Nout <= 32) bn = 32;
  else if (a.Nout <= 64) bn = 64;
  else if (a.Nout <= 80) bn = 80;
  else if (a.Nout <= 96) bn = 96;
  else if (a.Nout <= 128) bn = 128;
  else if (a.Nout > 192 && a.Nout <= 208) bn = 208;  // (BN 224 on 4 x 2 waves measured 2 % slower, r04)
  else {
    // fewest padded columns among the 128 / 192 / 224 tiles, the wider tile on ties
    // (measured: enhance_16 768->768 at 16x16 -24 %, the 8x8 576-channel layers +6 µs)
    int64_t best = -1;
    for (int c : {224, 192, 128}) {
      const int64_t pad = rup(a.Nout, c);
      if (best < 0 || pad < best) { best = pad; bn = c; }
    }
  }
  // (not for deep inputs: conv5_0's 206 -> 64 forward measured 0.43 -> 0.46 ms with it, against
  // add_128 0.59 -> 0.49 and conv0_res 0.35 -> 0.27)
  if (S == 2 && bn > 128) bn = 128;  // (the 1024-pixel halo leaves LDS for 128-row weight slices)
  const int bm = (S == 1 && halo_cfg512(bn) >= 0 && dtype != TPG_F32 && (int64_t)N * JH * JW >= 512 * 512 &&
                  JW >= 64 && cdiv(a.Nout, bn) == 1 && a.C <= 128) ? 512 : 256;
  const int HCAP = (bm == 512 || S == 2) ? 1024 : 5 * 128;
  int bth = 0, btw = 0, bimg = 0;
  int64_t bcost = -1;
  auto consider = [&](int th, int tw, int img) {
    if (th < 1 || tw < 1 || img < 1 || th * tw * img > bm) return;
    const int hpi = ((th - 1) * S + sy) * ((tw - 1) * S + sx);
    if ((int64_t)img * hpi > HCAP) return;
    const int64_t nsub = (int64_t)N * cdiv(JH, th) * cdiv(JW, tw);
    const int64_t blocks = (nsub + img - 1) / img;
    const int64_t cost = blocks * ((int64_t)bm * a.ntaps + (int64_t)img * hpi);
    if (bcost < 0 || cost < bcost) { bcost = cost; bth = th; btw = tw; bimg = img; }
  };
  if (JH * JW <= bm)
    for (int img = std::min(bm / (JH * JW), N); img >= 1; --img) consider(JH, JW, img);
  for (int tw : {JW, 64, 48, 40, 32, 24, 16, 8}) {
    if (tw > JW || tw > bm) continue;
    const int thmax = std::min(JH, bm / tw);
    if (thmax < 1) continue;
    consider(cdiv(JH, cdiv(JH, thmax)), tw, 1);
    // (stride 2: the tallest tile's halo may not fit; shorter ones, whole rows per block)
    if (S > 1)
      for (int th = thmax - 1; th >= 1 && th * tw * 2 >= bm / 2; --th) consider(th, tw, 1);
  }
  if (bcost < 0) return;
  if (a.Nout <= 32) bn = 32;
  else if (a.Nout <= 64) bn = 64;
  // (whole 16-pixel rows: the masked-gradient mode DMAs y into the halo buffer 16 pixels per
  // wave instruction)
  const int hcap = (int)rup((int64_t)bimg * ((bth - 1) * S + sy) * ((btw - 1) * S + sx), 16);
  const int hl = std::max(3, cdiv(hcap * 4, 512));
  const int cfg = bm == 512 ? halo_cfg512(bn) : halo_cfg(S == 2 ? 8 : hl, bn);
  if (cfg < 0) return;
  HaloArgs& h = P.h;
  const int ks_elems = half16(dtype) ? 32 : 16;
  h.A_H = a.A_H; h.A_W = a.A_W; h.C = a.C;
  h.nks = cdiv(a.C, ks_elems);
  h.ntaps = a.ntaps;
  // (16-bit: a last k-step with <= 16 live channels runs two taps per MFMA; never on the
  // pointwise kernel, which needs C % 32 == 0)
  h.half = (half16(dtype) && a.C % 32 != 0 && a.C % 32 <= 16) ? 1 : 0;
  h.dymin = dymin; h.dxmin = dxmin;
  h.TH = bth; h.TW = btw; h.IMG = bimg; h.SH = S; h.SW = S; h.dil = a.dil;
  h.HH = (bth - 1) * S + sy; h.HW = (btw - 1) * S + sx;
  h.hcap = hcap;
  for (int t = 0; t < a.ntaps; ++t) h.toff[t] = (a.dy[t] - dymin) * h.HW + (a.dx[t] - dxmin);
  h.pad_mode = a.pad_mode;
  h.N = N; h.JH = JH; h.JW = JW;
  h.tiles_h = cdiv(JH, bth); h.tiles_w = cdiv(JW, btw);
  h.fd_hp.init(h.HH * h.HW); h.fd_hw.init(h.HW);
  h.fd_tiles.init(h.tiles_h * h.tiles_w); h.fd_tilesw.init(h.tiles_w);
  h.fd_thw.init(bth * btw); h.fd_tw.init(btw);
  h.BN = bn; h.ntiles = cdiv(a.Nout, bn); h.Nout = a.Nout;
  h.oy0 = a.oy0; h.ox0 = a.ox0; h.osy = a.osy; h.osx = a.osx;
  // split over k-steps until the grid covers the chip (each split >= 4 pipeline steps)
  const int64_t base = (((int64_t)N * h.tiles_h * h.tiles_w + bimg - 1) / bimg) * h.ntiles;
  int ks = 1;
  constexpr int split_below = 256, split_to = 256, split_steps = 4;  // (swept in round 2: best)
  // (deterministic mode: no k-split at all, so a sample's outputs are summed in the same
  // order whatever the batch size — the DP run then matches the 1-GPU run at its global batch)
  if (base < split_below / cx.share && !cx.det) {
    const int kps_min = cdiv(split_steps, a.ntaps);
    ks = (int)std::min<int64_t>(cdiv(split_to / cx.share, (int)base), std::max(1, h.nks / kps_min));
  }
  if (cx.ks > 0 && !cx.det) ks = std::min(cx.ks, h.nks);  // (an autotuner's pick)
  // one tap (1x1 convs, stride 1 or 2) on whole 32-channel k-steps: the pointwise GEMM kernel,
  // whose 4-stage DMA ring hides the loads this kernel exposes every k-step when there is only
  // one tap per step; the largest of its tiles that still gives a chip's worth of blocks, and a
  // k split only for the few-block problems
  // Several taps: the same kernel (tap-shifted A rows by DMA, no reuse of a halo across taps)
  // where the halo grid is too small for the chip and would split K and the input is at most 256
  // channels deep (measured: local_20 128 ch 0.034 -> 0.021 ms, ResNet-50 l2 3x3 0.028 -> 0.018;
  // 512 / 768-channel maps slower, they keep the halo); desc.data_algo overrides (autotuner)
  const bool small_map =
      a.ntaps > 1 && (cx.algo == 2 || (cx.algo == 0 && base < split_below / cx.share && a.C <= 256));
  h.pw = 0;
  if ((a.ntaps == 1 || small_map) && a.dil <= 1 && half16(dtype) && a.C % 32 == 0 && bn % 64 == 0 && bn <= 192) {
    const int64_t M = (int64_t)N * JH * JW;
    int64_t bb = 0;
    for (int c = 1; c <= 4; ++c) {
      if (pw_tile_bn(c) > bn || bn % pw_tile_bn(c)) continue;
      const int64_t blocks = cdiv(M, pw_tile_bm(c)) * (int64_t)cdiv(a.Nout, pw_tile_bn(c));
      if (blocks > bb) { h.pw = c; bb = blocks; }
      if (blocks >= 240 / cx.share) { h.pw = c; bb = blocks; break; }
    }
    ks = 1;
    if (bb < 128 / cx.share && !cx.det) ks = (int)std::min<int64_t>(cdiv(256 / cx.share, (int)bb), h.nks / 8);
    if (cx.ks > 0 && !cx.det) ks = std::min(cx.ks, h.nks);
  }
  h.kps = cdiv(h.nks, std::max(ks, 1));
  h.ksplit = cdiv(h.nks, h.kps);
  P.halo = true;
  P.hcfg = cfg;
  P.hbm = bm;
  P.g_wp = P.wp_bytes;
  P.g_sk = P.sk_bytes;
  P.wp_bytes = (size_t)rup((int64_t)halo_wp_bytes(h.nks, h.ntaps, bn, h.ntiles, h.half), 256);
  P.pk.hnks = h.nks;
  P.pk.half = h.half;
  P.sk_bytes = h.ksplit > 1 ? (size_t)rup((int64_t)h.ksplit * a.M * a.Nout * 4, 256) : 0;
}

// ---- forward / input-gradient plans
// The full-kernel GEMM forms' geometry with a kernel of more than one tap; `in` (x, or dx in the
// input gradient) of a Conv2d / `out` (y, or g) of a ConvTranspose2d is the tensor whose
// (y, x, c) flatten into composite channels and must be dense NHWC.  Null: geometry alone.
bool composite(const tpg_conv_desc* d, const tpg_tensor* in, const tpg_tensor* out) {
  if (!gemm_form(d) || (d->kh == 1 && d->kw == 1)) return false;
  if (!d->transposed) return !in || dense_nhwc(*in, d->in_c, d->in_h, d->in_w);
  return !out || dense_nhwc(*out, d->out_c, d->out_h, d->out_w);
}

static size_t reflect_tmp_bytes(const tpg_conv_desc* d) {
  if (d->transposed || d->pad_mode != TPG_PAD_REFLECT) return 0;
  return (size_t)rup((int64_t)d->n * (d->in_h + d->pad_t + d->pad_b) * (d->in_w + d->pad_l + d->pad_r) *
                         rup(d->in_c, 8) * esize(d->dtype), 256);
}

// weight regions in plan order, the split-K slices behind them
static void place_regions(DataPlan* p) {
  size_t off = 0;
  for (Prob& P : p->v) {
    P.wp_off = off;
    off += P.region();
  }
  p->sk_off = off;
}

// The problems of (d, op) in the given form, their weight regions and the workspace they need.
//  operands   forward: A = x, N' = out_c over the output grid; input gradient: A = g, N' = in_c
//             over the input grid (reflect: the padded input, folded onto dx afterwards)
//  direct     Conv2d forward / ConvTranspose2d input gradient; else sub-pixel classes, or their
//             zero-insertion form when it gets the halo kernel
void plan_probs(const PlanCtx& cx, const tpg_conv_desc* d, bool fwd, bool comp, DataPlan* p) {
  const bool direct = fwd != (d->transposed != 0);
  const int Ca = fwd ? d->in_c : d->out_c, Cn = fwd ? d->out_c : d->in_c;
  p->d = *d;
  p->fwd = fwd; p->comp = comp;
  p->refl = !fwd && !comp && reflect_tmp_bytes(d) > 0;
  p->bias_mod = (fwd && comp && d->transposed) ? d->out_c : 0;
  p->v.clear();
  // operand sizes and pack modes, then the tile / split bookkeeping and the halo routing
  auto add = [&](Prob P, int C, int Nout, int nmode, int cmode) {
    P.a.C = C; P.a.Nout = Nout;
    P.a.A_H = comp ? 1 : fwd ? d->in_h : d->out_h;
    P.a.A_W = comp ? 1 : fwd ? d->in_w : d->out_w;
    P.pk.nmode = nmode; P.pk.cmode = cmode;
    if (comp) { P.pk.comp_kw = d->kw; P.pk.comp_c = direct ? Ca : Cn; }
    finish(P, cx, d->dtype, d->n * P.a.JH * P.a.JW);
    if (!comp) maybe_halo(P, cx, d->dtype, d->n);
    p->v.push_back(P);
  };
  const int GH = (fwd ? d->out_h : d->in_h) + (p->refl ? d->pad_t + d->pad_b : 0);
  const int GW = (fwd ? d->out_w : d->in_w) + (p->refl ? d->pad_l + d->pad_r : 0);
  const int pt = p->refl ? 0 : d->pad_t, pl = p->refl ? 0 : d->pad_l;
  if (comp) {  // e.g. dX[n][(y,x,ci)] = sum_co g[n][co] W[co][ci][y][x]
    Prob P = direct_prob(d->n, 1, 1, 1, 1, 1, 1, 0, 0);
    if (direct) add(P, d->kh * d->kw * Ca, Cn, 0, 2);
    else add(P, Ca, d->kh * d->kw * Cn, 2, 0);
  } else if (direct) {
    Prob P = direct_prob(d->n, GH, GW, d->kh, d->kw, d->stride_h, d->stride_w, d->pad_t, d->pad_l);
    P.a.pad_mode = d->pad_mode;
    add(P, Ca, Cn, 0, 1);
  } else {
    if (use_dilated(GH, GW, d->kh, d->kw, d->stride_h, d->stride_w, 0))
      add(dilated_prob(GH, GW, d->kh, d->kw, d->stride_h, pt, pl), Ca, Cn, 1, 0);
    if (p->v.empty() || !p->v[0].halo) {
      p->v.clear();
      for (const Prob& P : subpixel_probs(GH, GW, d->kh, d->kw, d->stride_h, d->stride_w, pt, pl)) add(P, Ca, Cn, 1, 0);
    }
  }
  p->tmp_bytes = p->refl ? reflect_tmp_bytes(d) : 0;
  size_t sk = 0;
  for (const Prob& P : p->v) sk = std::max(sk, std::max(P.sk_bytes, P.g_sk));
  place_regions(p);
  p->need = p->tmp_bytes + p->sk_off + sk;
}

// Workspace bytes of (d, op) whatever the tensors' layout: the larger of the two forms.
size_t data_workspace(const PlanCtx& cx, const tpg_conv_desc* d, bool fwd) {
  DataPlan p;
  size_t a = 0;
  if (!big_taps(d)) {
    plan_probs(cx, d, fwd, false, &p);
    a = p.need;
  }
  if (composite(d, nullptr, nullptr)) {
    plan_probs(cx, d, fwd, true, &p);
    a = std::max(a, p.need);
  }
  return a + 256;
}

static int64_t extent(const HaloArgs& h, const tpg_tensor& t) {
  return (int64_t)(h.N - 1) * std::abs(t.stride[0]) + (int64_t)(h.A_H - 1) * std::abs(t.stride[2]) +
         (int64_t)(h.A_W - 1) * std::abs(t.stride[3]) + h.C + 64;
}

// The finished plan of a call, or the status the launch would give: form, the kernel every
// problem finally runs on, masked mode, in_act in the epilogues, workspace layout.  Host
// arithmetic on the descriptor, dtypes, strides and pointer alignment only (no HIP call, no
// launch-group flush, no launch); run_data adds the pointers and launches.
int32_t plan_data(const PlanCtx& cx, const tpg_conv_desc* d, int32_t op, const DataLayouts& L, size_t ws_bytes,
                         DataPlan* p) {
  const bool fwd = op == TPG_OP_FWD, mask = op == TPG_OP_BWD_DATA_MASKED;
  const int dt = d->dtype;
  // masked mode: a stride-1 "same" Conv2d whose gy, y and g are 16-byte aligned rows, g laid out like y
  if (mask && !(!d->transposed && d->stride_h == 1 && d->stride_w == 1 && d->pad_mode == TPG_PAD_ZERO &&
                d->in_h == d->out_h && d->in_w == d->out_w && L.A && L.Y && L.M && L.G && L.A->dtype == dt &&
                L.M->dtype == dt && L.Y->dtype == dt && vec_ok(*L.A, dt) && vec_ok(*L.M, dt) && vec_ok(*L.G, dt) &&
                L.M->stride[0] == L.G->stride[0] && L.M->stride[2] == L.G->stride[2] &&
                L.M->stride[3] == L.G->stride[3]))
    return -31;
  const bool comp = fwd ? composite(d, L.A, L.Y) : composite(d, L.Y, L.A);
  if (mask && comp) return -31;
  if (!comp && big_taps(d)) return fail(-4, "%dx%d kernel: only the dense NHWC GEMM form is supported", d->kh, d->kw);
  if (L.packed && comp != composite(d, nullptr, nullptr))
    return fail(-21, "pre-packed weights assume a full-kernel GEMM; these tensors are not dense NHWC");
  plan_probs(cx, d, fwd, comp, p);
  p->packed = L.packed;
  if (comp && L.residual) return fail(-14, "residual not supported on a full-kernel conv");
  // DX_ACCUM: dx's entry values ride in as the epilogue's residual (read, then overwritten by
  // the same thread): dx = dgrad + dx
  if (!fwd && (d->flags & TPG_FLAG_DX_ACCUM) && (comp || p->refl))
    return fail(-32, "dx accumulation: zero-padded, non-GEMM-form geometries only");
  if (p->need > ws_bytes) return fail(-20, "workspace too small: %zu < %zu", ws_bytes, p->need);
  const bool vA = !L.A || vec_ok(*L.A, dt);
  std::vector<Prob>& v = p->v;
  if (mask) {  // the mask mode has no generic-kernel fallback
    // (the 512-row and stride-2 halo configs, ids >= 24, have no masked variant)
    if (v.size() != 1 || !v[0].halo || v[0].hcfg >= 24 || v[0].h.ntaps < 2 || !vA) return -31;
    if (extent(v[0].h, *L.A) >= (1ll << 31) || extent(v[0].h, *L.M) >= (1ll << 31)) return -31;
    if (!halo_accepts(v[0].h, v[0].hcfg, true)) return -31;
    v[0].h.pw = 0;
    p->masked = true;
  }
  for (Prob& P : v) {
    if (!P.halo || !L.A) continue;
    // the halo kernel takes 16-byte aligned channels-last rows and keeps 32-bit element
    // offsets into A
    if (!vA || extent(P.h, *L.A) >= (1ll << 31)) {
      if (L.packed) return fail(-21, "pre-packed weights assume the halo kernel; these tensors need the generic one");
      P.halo = false;
      P.wp_bytes = P.g_wp;
      P.sk_bytes = P.g_sk;
      place_regions(p);  // (its region shrinks to the generic kernel's; `need` keeps the halo plan's)
      continue;
    }
    // the pointwise kernel's 32-bit byte-extent / stride conditions are stricter than the element
    // counts above: where it would refuse, the halo kernel of the same plan and packed image runs
    P.h.a_sn = L.A->stride[0]; P.h.a_sh = L.A->stride[2]; P.h.a_sw = L.A->stride[3];
    if (P.h.pw > 0 && !pw_accepts(P.h, dt)) P.h.pw = 0;
    if (P.h.pw == 0 && !halo_accepts(P.h, P.hcfg, p->masked))
      return fail(-100, "halo conv: no kernel for config %d", P.hcfg);
  }
  // the producer's act' in the epilogues: all or nothing (a partial application could not be
  // completed by the caller's separate pass without applying it twice); X laid out like Y
  if (L.X && !p->refl) {
    const tpg_tensor &X = *L.X, &Y = *L.Y;
    bool ok = X.data && X.dtype == Y.dtype && X.stride[0] == Y.stride[0] && X.stride[2] == Y.stride[2] &&
              X.stride[3] == Y.stride[3] && X.stride[1] == 1 && vec_ok(X, dt) == vec_ok(Y, dt);
    for (const Prob& P : v) ok = ok && P.halo;
    p->xa = ok;
  }
  return 0;
}

}  // namespace tpg
