// C-ABI of libtpgan_hip.so (include/tpgan.h): the conv entry points validate, plan (tpg_plan.h)
// and run the plan's launch sequence (run_data, run_wgrad); the losses, fuser, maxout, Adam, SSD
// and landmark-front-end entry points validate and call their launcher.  Every entry point that launches calls
// group_sync() before its first launch and returns through hip_check / fail (tpg_internal.h).
#include "tpg_plan.h"
#include "../../include/tpgan.h"
#include <string.h>
#include <stdlib.h>

using namespace tpg;

extern "C" size_t tpg_conv2d_workspace(const tpg_conv_desc* d, int32_t op) {
  if (check_desc(d)) return 0;
  if (op == TPG_OP_FWD || op == TPG_OP_BWD_DATA) return data_workspace(plan_ctx(d), d, op == TPG_OP_FWD);
  return 256;  // bwd_filter accumulates straight into dw
}

// what follows the accumulation, the same for every problem of a call
struct Tail {
  const float* bias;
  tpg_tensor R, Y;
  float res_scale;
  int act;
  float slope;
  const void* XA;  // desc.in_act in the epilogues: x, read at Y's offsets
  int xa_act;
  float xa_slope;
};

// split-K finalize of `nslices` fp32 partial slices (1: one atomically accumulated slice)
static EpiArgs epi_args(const IgemmArgs& a, const float* ws, int nslices, int dtype, int bias_mod, const Tail& t) {
  EpiArgs ep;
  memset(&ep, 0, sizeof(ep));
  ep.ws = ws; ep.nslices = nslices; ep.slice = nslices > 1 ? (int64_t)a.M * a.Nout : 0;
  ep.M = a.M; ep.Nout = a.Nout; ep.JH = a.JH; ep.JW = a.JW;
  ep.Y = t.Y.data; ep.y_sn = t.Y.stride[0]; ep.y_sh = t.Y.stride[2]; ep.y_sw = t.Y.stride[3];
  ep.oy0 = a.oy0; ep.ox0 = a.ox0; ep.osy = a.osy; ep.osx = a.osx;
  ep.bias = t.bias; ep.bias_mod = bias_mod;
  ep.R = t.R.data; ep.r_sn = t.R.stride[0]; ep.r_sh = t.R.stride[2]; ep.r_sw = t.R.stride[3];
  ep.res_scale = t.res_scale; ep.act = t.act; ep.slope = t.slope; ep.dtype = dtype;
  ep.XA = t.XA; ep.xa_act = t.xa_act; ep.xa_slope = t.xa_slope;
  return ep;
}

// The launch sequence of a finished plan: per problem pack -> [zero split-K] -> kernel ->
// [finalize], then the reflect fold.  A, W, Y as in DataLayouts (W: fp32 weights, or the packed
// image of a WPACKED plan); R: the forward's residual, or dx itself under DX_ACCUM; M, G, X: the
// tensors the plan's masked mode / in_act epilogues read.  The halo kernel and its epilogue
// record into an open launch group; everything else flushes it first.
static int32_t run_data(const DataPlan& p, const tpg_tensor& A, const tpg_tensor& W, const float* bias,
                        const tpg_tensor& R, const tpg_tensor& Yc, const tpg_tensor* M, const tpg_tensor* G,
                        const tpg_tensor* X, char* ws, hipStream_t s) {
  const tpg_conv_desc* d = &p.d;
  const int dtype = d->dtype;
  tpg_tensor Y = Yc;
  if (p.refl) {  // gradient of the padded input into a dense NHWC temp, folded onto dx below
    const int PH = d->in_h + d->pad_t + d->pad_b, PW = d->in_w + d->pad_l + d->pad_r, Cp = (int)rup(d->in_c, 8);
    memset(&Y, 0, sizeof(Y));
    Y.data = ws; Y.dtype = dtype;
    Y.stride[0] = (int64_t)PH * PW * Cp; Y.stride[1] = 1; Y.stride[2] = (int64_t)PW * Cp; Y.stride[3] = Cp;
  }
  const Tail t = {bias, R, Y, p.fwd ? d->res_scale : R.data ? 1.f : 0.f, p.fwd ? d->act : TPG_ACT_NONE,
                  p.fwd ? d->slope : 0.f, p.xa ? X->data : nullptr, p.xa ? d->in_act : 0, p.xa ? d->in_slope : 0.f};
  const bool vA = vec_ok(A, dtype);
  char* wbase = p.packed ? reinterpret_cast<char*>(W.data) : ws + p.tmp_bytes;
  char* sk = ws + p.tmp_bytes + (p.packed ? 0 : p.sk_off);
  for (const Prob& P : p.v) {
    PackArgs k = P.pk;
    k.W = reinterpret_cast<const float*>(W.data);
    k.w_sa = W.stride[0]; k.w_sb = W.stride[1]; k.w_sr = W.stride[2]; k.w_ss = W.stride[3];
    k.Wp = wbase + P.wp_off;
    if (P.halo) {
      HaloArgs h = P.h;
      if (h.ntaps > 0 && !p.packed) {
        if (int32_t grc = group_sync()) return grc;
        int e = launch_pack_halo(k, h.nks, h.BN, h.ntiles, s);
        if (e) return hip_check(e, "pack_halo");
      }
      h.A = A.data; h.a_sn = A.stride[0]; h.a_sh = A.stride[2]; h.a_sw = A.stride[3];
      h.vec_ok = vA;
      h.Wp = k.Wp;
      h.Y = Y.data; h.y_sn = Y.stride[0]; h.y_sh = Y.stride[2]; h.y_sw = Y.stride[3];
      h.bias = bias;
      h.R = R.data; h.r_sn = R.stride[0]; h.r_sh = R.stride[2]; h.r_sw = R.stride[3];
      h.res_scale = t.res_scale; h.act = t.act; h.slope = t.slope;
      h.ws = h.ksplit > 1 ? reinterpret_cast<float*>(sk) : nullptr;
      h.yvec = vec_ok(Y, dtype);
      h.rvec = R.data ? vec_ok(R, dtype) : 0;
      h.wvec = P.a.Nout % 4 == 0;
      if (p.masked) {
        h.M = M->data; h.m_sn = M->stride[0]; h.m_sh = M->stride[2]; h.m_sw = M->stride[3];
        h.G = G->data; h.mact = d->act; h.mslope = d->slope;
      }
      h.XA = t.XA; h.xa_act = t.xa_act; h.xa_slope = t.xa_slope;
      int e = do_halo(h, dtype, P.hcfg, s, p.masked);
      if (e) return hip_check(e, "halo conv");
      if (h.ksplit > 1) {
        e = do_epilogue(epi_args(P.a, h.ws, h.ksplit, dtype, 0, t), s);
        if (e) return hip_check(e, "halo epilogue");
      }
      continue;
    }
    if (int32_t grc = group_sync()) return grc;
    IgemmArgs a = P.a;
    if (a.nunits > 0 && !p.packed) {
      int e = launch_pack(k, s);
      if (e) return hip_check(e, "pack");
    }
    a.A = A.data; a.a_sn = A.stride[0]; a.a_sh = A.stride[2]; a.a_sw = A.stride[3];
    a.vec_ok = vA;
    a.Wp = k.Wp;
    a.Y = Y.data; a.y_sn = Y.stride[0]; a.y_sh = Y.stride[2]; a.y_sw = Y.stride[3];
    a.bias = bias; a.bias_mod = p.bias_mod;
    a.R = R.data; a.r_sn = R.stride[0]; a.r_sh = R.stride[2]; a.r_sw = R.stride[3];
    a.res_scale = t.res_scale; a.act = t.act; a.slope = t.slope;
    a.ws = nullptr;
    if (a.ksplit > 1) {
      a.ws = reinterpret_cast<float*>(sk);
      hipError_t e = hipMemsetAsync(sk, 0, (size_t)a.M * a.Nout * 4, s);
      if (e) return hip_check((int)e, "hipMemsetAsync");
    }
    int e = launch_igemm(a, dtype, P.cfg, s);
    if (e) return hip_check(e, "igemm");
    if (a.ksplit > 1) {
      e = launch_epilogue(epi_args(a, a.ws, 1, dtype, p.bias_mod, t), s);
      if (e) return hip_check(e, "epilogue");
    }
  }
  if (!p.refl) return 0;
  if (int32_t grc = group_sync()) return grc;
  return hip_check(launch_reflect_fold(d->n, d->in_c, d->in_h, d->in_w, d->pad_t, d->pad_b, d->pad_l, d->pad_r, Y, Yc, s),
                   "reflect_fold");
}

// the tensors every forward / input-gradient call needs: A, Y and fp32 (or pre-packed) weights
static int32_t check_data_call(const tpg_conv_desc* d, const tpg_tensor& A, const char* an, const tpg_tensor& Y,
                               const char* yn, const tpg_tensor& w) {
  int32_t rc;
  if ((rc = check_tensor(A, d->dtype, an)) || (rc = check_tensor(Y, d->dtype, yn))) return rc;
  if (!w.data || (w.dtype != TPG_F32 && !(d->flags & TPG_FLAG_WPACKED))) return fail(-13, "weight must be fp32");
  return 0;
}

// ------------------------------------------------------------ pre-packed weights --
// The packed image of (d, op) is the weight part of the op's workspace for the plan the
// op picks on 16-byte aligned channels-last tensors: one region per problem, in plan order.
static void pack_plan(const PlanCtx& cx, const tpg_conv_desc* d, int32_t op, DataPlan* p) {
  plan_probs(cx, d, op == TPG_OP_FWD, composite(d, nullptr, nullptr), p);
}

extern "C" size_t tpg_conv2d_packed_bytes(const tpg_conv_desc* d, int32_t op) {
  if (check_desc(d) || (op != TPG_OP_FWD && op != TPG_OP_BWD_DATA)) return 0;
  DataPlan p;
  pack_plan(plan_ctx(d), d, op, &p);
  return packed_bytes(p);
}

extern "C" size_t tpg_pack_job_bytes(void) { return sizeof(PackJob); }

extern "C" int32_t tpg_conv2d_pack_jobs(const tpg_conv_desc* d, int32_t op, tpg_tensor w, void* wp, void* jobs,
                                        int32_t max_jobs) {
  int32_t rc = check_desc(d);
  if (rc) return rc;
  if (op != TPG_OP_FWD && op != TPG_OP_BWD_DATA) return fail(-2, "pack: op must be fwd or bwd_data");
  if (!w.data || w.dtype != TPG_F32 || !wp || !jobs) return fail(-10, "pack: NULL / non-fp32 weight");
  DataPlan p;
  pack_plan(plan_ctx(d), d, op, &p);
  PackJob* out = reinterpret_cast<PackJob*>(jobs);
  int n = 0;
  for (const Prob& P : p.v) {
    if (!(P.halo ? P.h.ntaps > 0 : P.a.nunits > 0)) continue;
    if (n >= max_jobs) return fail(-22, "pack: more than %d jobs", max_jobs);
    PackJob& j = out[n++];
    memset(&j, 0, sizeof(j));
    j.k = P.pk;
    j.k.W = reinterpret_cast<const float*>(w.data);
    j.k.w_sa = w.stride[0]; j.k.w_sb = w.stride[1]; j.k.w_sr = w.stride[2]; j.k.w_ss = w.stride[3];
    j.k.Wp = reinterpret_cast<char*>(wp) + P.wp_off;
    if (P.halo) {
      j.kind = 1;
      j.nks = P.h.nks; j.bn = P.h.BN; j.bnl = (P.h.BN + 127) / 128 * 128; j.ntiles = P.h.ntiles;
      j.items = halo_steps(j.nks, j.k.ntaps, P.h.half) * j.ntiles * j.bnl * 4;
    } else {
      j.kind = 0;
      j.items = j.k.Npad * j.k.nunits;
    }
    j.nblocks = cdiv(j.items, 256 * TPG_PACK_GROUPS);
  }
  return n;
}

extern "C" int64_t tpg_pack_prepare(void* jobs, int32_t n) {
  PackJob* j = reinterpret_cast<PackJob*>(jobs);
  int64_t b = 0;
  for (int i = 0; i < n; ++i) {
    j[i].first_block = (int)b;
    b += j[i].nblocks;
  }
  return b;
}

extern "C" int32_t tpg_pack_run(const void* jobs_dev, int32_t n, int64_t nblocks, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  if (n <= 0) return 0;
  if (!jobs_dev || nblocks <= 0 || nblocks >= (1ll << 31)) return fail(-2, "pack_run: bad batch");
  return hip_check(launch_pack_many(reinterpret_cast<const PackJob*>(jobs_dev), n, (int)nblocks, (hipStream_t)stream),
                   "pack_run");
}

static const tpg_tensor g_none = {};

extern "C" int32_t tpg_conv2d_fwd(const tpg_conv_desc* d, tpg_tensor x, tpg_tensor w, const float* bias,
                                  tpg_tensor residual, tpg_tensor y, void* ws, size_t ws_bytes, tpg_stream_t stream) {
  int32_t rc = check_desc(d);
  if (rc) return rc;
  if ((rc = check_data_call(d, x, "x", y, "y", w))) return rc;
  if (residual.data && (rc = check_tensor(residual, d->dtype, "residual"))) return rc;
  DataLayouts L;
  L.A = &x; L.Y = &y; L.residual = residual.data != nullptr; L.packed = d->flags & TPG_FLAG_WPACKED;
  DataPlan p;
  if ((rc = plan_data(plan_ctx(d), d, TPG_OP_FWD, L, ws_bytes, &p))) return rc;
  return run_data(p, x, w, bias, residual, y, nullptr, nullptr, nullptr, reinterpret_cast<char*>(ws), (hipStream_t)stream);
}

extern "C" int32_t tpg_conv2d_bwd_data(const tpg_conv_desc* d, tpg_tensor g, tpg_tensor w, tpg_tensor dx, void* ws,
                                       size_t ws_bytes, tpg_stream_t stream) {
  int32_t rc = check_desc(d);
  if (rc) return rc;
  if (d->in_act != TPG_ACT_NONE) return fail(-33, "bwd_data: desc.in_act needs x (tpg_conv2d_bwd)");
  if ((rc = check_data_call(d, g, "g", dx, "dx", w))) return rc;
  DataLayouts L;
  L.A = &g; L.Y = &dx; L.packed = d->flags & TPG_FLAG_WPACKED;
  DataPlan p;
  if ((rc = plan_data(plan_ctx(d), d, TPG_OP_BWD_DATA, L, ws_bytes, &p))) return rc;
  return run_data(p, g, w, nullptr, (d->flags & TPG_FLAG_DX_ACCUM) ? dx : g_none, dx, nullptr, nullptr, nullptr,
                  reinterpret_cast<char*>(ws), (hipStream_t)stream);
}

extern "C" int32_t tpg_conv2d_data_plan(const tpg_conv_desc* d, int32_t op, tpg_tensor a, tpg_tensor y, tpg_tensor m,
                                        tpg_tensor g, tpg_tensor x, size_t ws_bytes, tpg_data_plan* out) {
  if (!out) return fail(-1, "null plan");
  int32_t rc = check_desc(d);
  if (rc) return rc;
  if (op != TPG_OP_FWD && op != TPG_OP_BWD_DATA && op != TPG_OP_BWD_DATA_MASKED)
    return fail(-2, "data plan: op must be fwd, bwd_data or bwd_data_masked");
  if ((rc = check_tensor(a, d->dtype, "a")) || (rc = check_tensor(y, d->dtype, "y"))) return rc;
  const PlanCtx cx = plan_ctx(d);
  DataLayouts L;
  L.A = &a; L.Y = &y; L.packed = d->flags & TPG_FLAG_WPACKED;
  if (op == TPG_OP_BWD_DATA_MASKED) { L.M = &m; L.G = &g; }
  if (op != TPG_OP_FWD && d->in_act != TPG_ACT_NONE) L.X = &x;
  DataPlan p;
  if ((rc = plan_data(cx, d, op, L, ws_bytes, &p)))
    return rc == -31 ? fail(-31, "masked input-gradient mode does not apply to this call") : rc;
  if (p.v.size() > TPG_DATA_MAX_PROBS) return fail(-22, "data plan: more than %d problems", TPG_DATA_MAX_PROBS);
  memset(out, 0, sizeof(*out));
  out->nprobs = (int32_t)p.v.size();
  out->flags = (p.comp ? TPG_DATA_COMPOSITE : 0) | (p.v[0].a.dil > 1 ? TPG_DATA_DILATED : 0) |
               (p.refl ? TPG_DATA_REFLECT_FOLD : 0) | (p.masked ? TPG_DATA_MASKED : 0) | (p.xa ? TPG_DATA_IN_ACT : 0);
  out->ws_bytes = data_workspace(cx, d, p.fwd);
  out->packed_bytes = packed_bytes(p);
  out->tmp_bytes = p.tmp_bytes;
  out->sk_off = p.tmp_bytes + (p.packed ? 0 : p.sk_off);
  for (size_t i = 0; i < p.v.size(); ++i) {
    const Prob& P = p.v[i];
    tpg_data_prob& o = out->prob[i];
    o.taps = P.a.ntaps;
    o.wp_off = (p.packed ? 0 : p.tmp_bytes) + P.wp_off;
    o.wp_bytes = P.region();
    o.sk_bytes = P.sk_bytes;
    if (P.halo) {
      const HaloArgs& h = P.h;
      o.kernel = h.pw > 0 ? TPG_DATA_POINTWISE : TPG_DATA_HALO;
      o.cfg = P.hcfg; o.th = h.TH; o.tw = h.TW; o.img = h.IMG; o.bn = h.BN; o.rows = P.hbm; o.halo_px = h.hcap;
      o.ksteps = h.nks; o.ksplit = h.ksplit; o.kps = h.kps; o.paired = h.half; o.pw_tile = h.pw;
    } else {
      o.kernel = TPG_DATA_GENERIC;
      o.cfg = P.cfg; o.bn = igemm_cfg_bn(P.cfg); o.rows = igemm_cfg_bm(P.cfg);
      o.ksteps = P.a.nunits / (half16(d->dtype) ? 4 : 2); o.ksplit = P.a.ksplit; o.kps = P.a.kt_per_split;
    }
  }
  return 0;
}

// The launch sequence of a plan; dbias may be null.  The flat kernel records into an open
// launch group (do_wgrad2); the others flush it first.
static int32_t run_wgrad(WgradPlan& p, const tpg_tensor& x, const tpg_tensor& g, const tpg_tensor& dw, float* dbias,
                         hipStream_t stream) {
  if (!p.sums_bias) dbias = nullptr;
  if (p.kernel == TPG_WGRAD_ROW_HALO || p.kernel == TPG_WGRAD_IMAGE_HALO) {
    p.rh.P = g.data; p.rh.Q = x.data;
    p.rh.dW = reinterpret_cast<float*>(dw.data);
    p.rh.dbias = dbias;
    if (int32_t grc = group_sync()) return grc;
    return hip_check(launch_wgrad_rh(p.rh, stream), "wgrad_rh");
  }
  p.a.P = p.p_is_x ? x.data : g.data;
  p.a.Q = p.p_is_x ? g.data : x.data;
  p.a.dW = reinterpret_cast<float*>(dw.data);
  if (p.kernel == TPG_WGRAD_FLAT) {
    p.a.dbias = dbias;
    return hip_check(do_wgrad2(p.a, x.dtype, p.cfg, p.bm, p.bn, stream), "wgrad2");
  }
  if (int32_t grc = group_sync()) return grc;
  return hip_check(launch_wgrad(p.a, x.dtype, p.cfg, stream), "wgrad");
}

// Weight gradient; with dbias (Conv2d only: the pixel-grid operand is g) the bias gradient is
// summed by the same launch where the kernel supports it (*bias_done), else left to the caller.
static int32_t bwd_filter_run(const tpg_conv_desc* d, const tpg_tensor& x, const tpg_tensor& g, const tpg_tensor& dw,
                               float* dbias, bool* bias_done, tpg_stream_t stream) {
  *bias_done = false;
  WgradPlan p;
  int32_t rc = plan_bwd_filter(d, x, g, dw, &p);
  if (rc) return rc;
  rc = run_wgrad(p, x, g, dw, dbias, (hipStream_t)stream);
  *bias_done = rc == 0 && dbias != nullptr && p.sums_bias;
  return rc;
}

extern "C" int32_t tpg_conv2d_wgrad_plan(const tpg_conv_desc* d, tpg_tensor x, tpg_tensor g, tpg_tensor dw,
                                         tpg_wgrad_plan* out) {
  if (!out) return fail(-1, "null plan");
  WgradPlan p;
  const int32_t rc = plan_bwd_filter(d, x, g, dw, &p);
  if (rc) return rc;
  const bool rh = p.kernel == TPG_WGRAD_ROW_HALO || p.kernel == TPG_WGRAD_IMAGE_HALO;
  out->kernel = p.kernel; out->cfg = p.cfg; out->tile_m = p.bm; out->tile_n = p.bn;
  out->splits = rh ? p.rh.ksplit : p.a.ksplit;
  out->per_split = rh ? p.rh.kt_per_split : p.a.pix_per_split;
  out->tiles = p.tiles;
  out->taps_per_block = p.rh.nr * p.rh.nt;
  out->bias_share = rh ? p.rh.bshare : p.a.bshare;
  out->flags = (p.sums_bias ? TPG_WGRAD_SUMS_BIAS : 0) | (p.a.bflat ? TPG_WGRAD_BFLAT : 0) |
               (p.a.fastp ? TPG_WGRAD_FASTP : 0) | (p.a.fastq ? TPG_WGRAD_FASTQ : 0) |
               (p.rh.skip ? TPG_WGRAD_SKIP : 0) |
               (p.kernel == TPG_WGRAD_FLAT && p.a.bflat ? TPG_WGRAD_GROUPED : 0);
  return 0;
}

extern "C" int32_t tpg_conv2d_bwd_filter(const tpg_conv_desc* d, tpg_tensor x, tpg_tensor g, tpg_tensor dw, void* ws,
                                         size_t ws_bytes, tpg_stream_t stream) {
  (void)ws; (void)ws_bytes;
  bool bias_done;
  return bwd_filter_run(d, x, g, dw, nullptr, &bias_done, stream);
}

// Fused per-layer backward (SURVEY.md §8b tpg_conv2d_bwd): g = gy * act'(y), dx, dw, dbias.
extern "C" int32_t tpg_conv2d_bwd(const tpg_conv_desc* d, tpg_tensor x, tpg_tensor w, tpg_tensor y, tpg_tensor gy,
                                  tpg_tensor g, tpg_tensor dx, tpg_tensor dw, float* dbias, void* ws, size_t ws_bytes,
                                  tpg_stream_t stream) {
  int32_t rc = check_desc(d);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (!gy.data) return fail(-10, "conv2d_bwd: gy is NULL");
  const bool has_act = d->act != TPG_ACT_NONE;
  if (has_act && !y.data) return fail(-10, "conv2d_bwd: y is NULL with an activation");
  // without an activation g IS gy (when it already has the compute dtype)
  // (16-byte aligned channels-last rows: the weight-gradient DMA kernels read g as it is)
  const bool g_is_gy = !has_act && gy.dtype == d->dtype && vec_ok(gy, d->dtype);
  if (!g_is_gy && (rc = check_tensor(g, d->dtype, "g"))) return rc;
  const tpg_tensor& G = g_is_gy ? gy : g;
  bool bias_done = false;
  const bool acc = dx.data && (d->flags & TPG_FLAG_DX_ACCUM);
  // desc.in_act: dx leaves as dx * in_act'(x) (the producer's activation backward)
  const bool xact = dx.data && d->in_act != TPG_ACT_NONE;
  if (xact) {
    if (d->in_act < TPG_ACT_NONE || d->in_act > TPG_ACT_RELU6) return fail(-2, "conv2d_bwd: bad in_act %d", d->in_act);
    if ((rc = check_tensor(x, d->dtype, "x")) || (rc = check_tensor(dx, d->dtype, "dx"))) return rc;
  }
  if (acc && (composite(d, nullptr, nullptr) || (!d->transposed && d->pad_mode == TPG_PAD_REFLECT)))
    return fail(-32, "dx accumulation: zero-padded, non-GEMM-form geometries only");
  // The input gradient is planned before anything is launched, so a status (-21: pre-packed
  // weights these tensors cannot use) comes back before the bias gradient was added anywhere and
  // the caller's retry with fp32 weights adds nothing twice.  Masked mode where the plan has it:
  // the activation' applied while the halo is staged, g written on the way
  // (round 1 measured 42.1 ms/step with maps up to 64 x 64, 42.5 with every map, 43.0 with
  // none; after the 512-row and stride-2 tiles -- which have no masked variant and take the
  // separate pass -- every map measured 37.39 vs 37.54 / 37.56 at 64 x 64)
  DataPlan dp;
  if (dx.data) {
    if ((rc = check_data_call(d, G, "g", dx, "dx", w))) return rc;
    const PlanCtx cx = plan_ctx(d);
    DataLayouts L;
    L.A = &gy; L.Y = &dx; L.M = &y; L.G = &g; L.X = xact ? &x : nullptr; L.packed = d->flags & TPG_FLAG_WPACKED;
    rc = g_is_gy ? -31 : plan_data(cx, d, TPG_OP_BWD_DATA_MASKED, L, ws_bytes, &dp);
    if (rc == -31) {
      L.A = &G;
      rc = plan_data(cx, d, TPG_OP_BWD_DATA, L, ws_bytes, &dp);
    }
    if (rc) return rc;
  }
  // otherwise the activation backward pass materialises g (and sums the bias when there is
  // no weight gradient: with one, the weight-gradient launch sums it, the same order whether
  // the caller runs the weight gradient here or as a second call on another stream)
  if (!g_is_gy && !dp.masked) {
    // (ConvTranspose2d: its weight-gradient kernels never take the bias -- it would cost a
    // separate column-sum launch, so this pass keeps it)
    float* db = (dw.data && !d->transposed) ? nullptr : dbias;
    rc = hip_check(do_act_bwd(d->n, d->out_c, d->out_h, d->out_w, d->act, d->slope, gy, y, g, db, s),
                   "act_bwd");
    if (rc) return rc;
    bias_done = db != nullptr;
  }
  if (dx.data && (rc = run_data(dp, dp.masked ? gy : G, w, nullptr, acc ? dx : g_none, dx, &y, &g, &x,
                                reinterpret_cast<char*>(ws), s)))
    return rc;
  if (xact && !dp.xa) {  // (plans whose epilogue cannot take it: one in-place pass over dx)
    rc = hip_check(do_act_bwd(d->n, d->in_c, d->in_h, d->in_w, d->in_act, d->in_slope, dx, x, dx, nullptr, s),
                   "act_bwd (in_act)");
    if (rc) return rc;
  }
  // 3. the weight gradient, summing the bias gradient in the same launch where it can
  if (dw.data) {
    bool b = false;
    if ((rc = bwd_filter_run(d, x, G, dw, bias_done ? nullptr : dbias, &b, stream))) return rc;
    bias_done = bias_done || b;
  }
  if (dbias && !bias_done) {
    if (int32_t grc = group_sync()) return grc;
    return hip_check(launch_colsum(d->n, d->out_c, d->out_h, d->out_w, G, dbias, s), "colsum");
  }
  return 0;
}

// ------------------------------------------------------------------ fused G losses --
static constexpr size_t LOSS_WS = 512 * TPG_L1_MAX_SEGS * sizeof(float);  // (tpg_losses.hip LS_BLOCKS)
extern "C" size_t tpg_loss_workspace(void) { return LOSS_WS; }

static int32_t check_loss_tensor(const tpg_tensor& t, const char* what) {
  if (!t.data) return fail(-10, "%s is NULL", what);
  if (t.dtype != TPG_F32 && t.dtype != TPG_BF16 && t.dtype != TPG_F16) return fail(-11, "%s: bad dtype %d", what, t.dtype);
  return 0;
}

extern "C" int32_t tpg_image_losses_fwd(int32_t n, int32_t c, int32_t h, int32_t w, tpg_tensor x, tpg_tensor r,
                                        float w_pix, float w_sym, float w_tv, float* ws, size_t ws_bytes, float* out,
                                        tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  int32_t rc;
  if (n < 1 || c < 1 || h < 1 || w < 1) return fail(-2, "image_losses: empty shape");
  if ((rc = check_loss_tensor(x, "x")) || (rc = check_loss_tensor(r, "r"))) return rc;
  if (!ws || ws_bytes < LOSS_WS || !out) return fail(-20, "image_losses: workspace / out");
  return hip_check(launch_image_losses(n, c, h, w, x, r, w_pix, w_sym, w_tv, ws, nullptr, out, nullptr,
                                       (hipStream_t)stream), "image_losses");
}

extern "C" int32_t tpg_image_losses_bwd(int32_t n, int32_t c, int32_t h, int32_t w, tpg_tensor x, tpg_tensor r,
                                        float w_pix, float w_sym, float w_tv, const float* gout, tpg_tensor dx,
                                        tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  int32_t rc;
  if (n < 1 || c < 1 || h < 1 || w < 1) return fail(-2, "image_losses: empty shape");
  if ((rc = check_loss_tensor(x, "x")) || (rc = check_loss_tensor(r, "r")) || (rc = check_loss_tensor(dx, "dx")))
    return rc;
  if (!gout) return fail(-10, "image_losses: gout is NULL");
  return hip_check(launch_image_losses(n, c, h, w, x, r, w_pix, w_sym, w_tv, nullptr, gout, nullptr, &dx,
                                       (hipStream_t)stream), "image_losses_bwd");
}

static int32_t check_l1_segs(int32_t nseg, const tpg_l1_seg* segs, bool bwd) {
  if (nseg < 1 || nseg > TPG_L1_MAX_SEGS || !segs) return fail(-2, "l1_set: 1..%d segments", TPG_L1_MAX_SEGS);
  for (int k = 0; k < nseg; ++k) {
    const tpg_l1_seg& s = segs[k];
    int32_t rc;
    if (s.n < 1 || s.c < 1 || s.h < 1 || s.w < 1) return fail(-2, "l1_set: segment %d empty", k);
    if ((rc = check_loss_tensor(s.a, "a")) || (rc = check_loss_tensor(s.b, "b"))) return rc;
    if (bwd && s.da.data && (rc = check_loss_tensor(s.da, "da"))) return rc;
  }
  return 0;
}

extern "C" int32_t tpg_l1_set_fwd(int32_t nseg, const tpg_l1_seg* segs, float* ws, size_t ws_bytes, float* out,
                                  tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  int32_t rc = check_l1_segs(nseg, segs, false);
  if (rc) return rc;
  if (!ws || ws_bytes < LOSS_WS || !out) return fail(-20, "l1_set: workspace / out");
  return hip_check(launch_l1_set(nseg, segs, ws, nullptr, out, false, (hipStream_t)stream), "l1_set");
}

extern "C" int32_t tpg_l1_set_bwd(int32_t nseg, const tpg_l1_seg* segs, const float* gout, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  int32_t rc = check_l1_segs(nseg, segs, true);
  if (rc) return rc;
  if (!gout) return fail(-10, "l1_set: gout is NULL");
  return hip_check(launch_l1_set(nseg, segs, nullptr, gout, nullptr, true, (hipStream_t)stream), "l1_set_bwd");
}

extern "C" int32_t tpg_act_bwd(int32_t n, int32_t c, int32_t h, int32_t w, int32_t act, float slope, tpg_tensor gy,
                               tpg_tensor y, tpg_tensor g, float* dbias, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  if (!gy.data || !g.data || (act != TPG_ACT_NONE && !y.data)) return fail(-10, "act_bwd: NULL tensor");
  return hip_check(launch_act_bwd(n, c, h, w, act, slope, gy, y, g, dbias, (hipStream_t)stream), "act_bwd");
}

extern "C" int32_t tpg_copy4d(int32_t n, int32_t c, int32_t h, int32_t w, tpg_tensor in, tpg_tensor out,
                              tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  if (!in.data || !out.data) return fail(-10, "copy4d: NULL tensor");
  if ((int64_t)n * c * h * w == 0) return 0;
  return hip_check(launch_copy4d(n, c, h, w, in, out, (hipStream_t)stream), "copy4d");
}

extern "C" int32_t tpg_fold_taps(int32_t n, int32_t c, int32_t h, int32_t w, int32_t fh, int32_t fw, int32_t sh,
                                 int32_t sw, int32_t pt, int32_t pl, int32_t oh, int32_t ow, tpg_tensor x, tpg_tensor y,
                                 int32_t backward, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  if (!x.data || !y.data) return fail(-10, "fold_taps: NULL tensor");
  if (fh < 1 || fw < 1 || sh < 1 || sw < 1 || n < 0 || c < 1 || (int64_t)fh * fw * c > 4096)
    return fail(-2, "fold_taps: bad geometry");
  if ((int64_t)n * (backward ? (int64_t)h * w * c : (int64_t)oh * ow * fh * fw * c) == 0) return 0;
  return hip_check(launch_fold_taps(n, c, h, w, fh, fw, sh, sw, pt, pl, oh, ow, x, y, backward, (hipStream_t)stream),
                   "fold_taps");
}

extern "C" int32_t tpg_local_fuse_fwd(int32_t n, int32_t c, int32_t out_h, int32_t out_w, const tpg_tensor* parts,
                                      const int32_t* ph, const int32_t* pw, const int32_t* top, const int32_t* left,
                                      tpg_tensor y, uint8_t* argmax, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  for (int k = 0; k < 4; ++k)
    if (!parts[k].data) return fail(-10, "local_fuse: part %d NULL", k);
  return hip_check(launch_fuse_fwd(n, c, out_h, out_w, parts, ph, pw, top, left, y, argmax, (hipStream_t)stream),
                   "local_fuse_fwd");
}

extern "C" int32_t tpg_local_fuse_bwd(int32_t n, int32_t c, int32_t out_h, int32_t out_w, tpg_tensor gy,
                                      const uint8_t* argmax, const tpg_tensor* dparts, const int32_t* ph,
                                      const int32_t* pw, const int32_t* top, const int32_t* left, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  if (!argmax || !gy.data) return fail(-10, "local_fuse_bwd: NULL");
  return hip_check(launch_fuse_bwd(n, c, out_h, out_w, gy, argmax, dparts, ph, pw, top, left, (hipStream_t)stream),
                   "local_fuse_bwd");
}

extern "C" int32_t tpg_maxout2_fwd(int32_t b, int32_t m, tpg_tensor x, tpg_tensor y, uint8_t* argmax,
                                   tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  return hip_check(launch_maxout_fwd(b, m, x, y, argmax, (hipStream_t)stream), "maxout_fwd");
}

extern "C" int32_t tpg_maxout2_bwd(int32_t b, int32_t m, tpg_tensor gy, const uint8_t* argmax, tpg_tensor dx,
                                   tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  return hip_check(launch_maxout_bwd(b, m, gy, argmax, dx, (hipStream_t)stream), "maxout_bwd");
}

extern "C" int32_t tpg_adam(int64_t numel, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                            float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                            float grad_scale, float* state, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  if (numel < 0) return fail(-2, "adam: numel must be >= 0");
  if (numel == 0 && step < 0) return 0;
  if (!state) return fail(-10, "adam: NULL state");
  if (numel > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)) return fail(-10, "adam: NULL pointer");
  const int rc = launch_adam(numel, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step,
                               grad_scale, state, (hipStream_t)stream);
  if (rc == -1) return fail(-15, "adam: buffers must be 4-byte aligned, at one offset inside 16 bytes");
  return hip_check(rc, "adam");
}

extern "C" int32_t tpg_grad_check(int64_t numel, const float* grad, float* state, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  if (!grad || !state) return fail(-10, "grad_check: NULL pointer");
  const int rc = launch_grad_check(numel, grad, state, (hipStream_t)stream);
  if (rc == -1) return fail(-15, "grad_check: gradient buffer must be 16-byte aligned");
  return hip_check(rc, "grad_check");
}

// ---- SSD landmark head (MobileNetV2.py:342-649; tpg_ssd.hip)
static int32_t check_ssd(int32_t B, int32_t n, int32_t C, const void* pred, const void* cls, const char* who) {
  if (B < 1 || n < 1 || n > TPG_SSD_MAXN || C < 5) return fail(-2, "%s: B %d, n %d (1..%d), C %d (>= 5)", who, B, n,
                                                              TPG_SSD_MAXN, C);
  if (!pred || !cls) return fail(-10, "%s: NULL input", who);
  if (((uintptr_t)pred | (uintptr_t)cls) % 4) return fail(-15, "%s: inputs must be 4-byte aligned", who);
  return 0;
}

extern "C" int32_t tpg_ssd_loss_fwd(int32_t B, int32_t n, int32_t C, const float* pred, const float* cls,
                                    const float* truth, float width, float height, int32_t k, double ratio_nb,
                                    float alpha, float beta, const float* keys, int32_t* labels, uint8_t* sel,
                                    float* terms, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  int32_t rc = check_ssd(B, n, C, pred, cls, "ssd_loss_fwd");
  if (rc) return rc;
  if (!truth || !keys || !labels || !sel || !terms) return fail(-10, "ssd_loss_fwd: NULL buffer");
  if (!(width > 0.f) || !(height > 0.f)) return fail(-2, "ssd_loss_fwd: image size must be positive");
  if (k < 1 || k > n) return fail(-2, "ssd_loss_fwd: k = %d outside 1..%d", k, n);
  return hip_check(launch_ssd_loss_fwd(B, n, C, k, pred, cls, truth, width, height, ratio_nb, alpha, beta, keys, labels,
                                       sel, terms, (hipStream_t)stream), "ssd_loss_fwd");
}

extern "C" int32_t tpg_ssd_loss_bwd(int32_t B, int32_t n, int32_t C, const float* pred, const float* cls,
                                    const float* truth, float width, float height, float alpha, float beta,
                                    const int32_t* labels, const uint8_t* sel, const float* terms, const float* gout,
                                    float* dloc, float* dcls, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  int32_t rc = check_ssd(B, n, C, pred, cls, "ssd_loss_bwd");
  if (rc) return rc;
  if (!truth || !labels || !sel || !terms || !gout || !dloc || !dcls) return fail(-10, "ssd_loss_bwd: NULL buffer");
  if (!(width > 0.f) || !(height > 0.f)) return fail(-2, "ssd_loss_bwd: image size must be positive");
  return hip_check(launch_ssd_loss_bwd(B, n, C, pred, cls, truth, width, height, alpha, beta, labels, sel, terms, gout,
                                       dloc, dcls, (hipStream_t)stream), "ssd_loss_bwd");
}

extern "C" int32_t tpg_ssd_decode(int32_t B, int32_t n, int32_t C, const float* loc, const float* cls, float conf,
                                  float nms_thr, int32_t top_k, int32_t* keep, float* score, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  int32_t rc = check_ssd(B, n, C, loc, cls, "ssd_decode");
  if (rc) return rc;
  if (top_k < 1 || top_k > 64) return fail(-2, "ssd_decode: top_k %d outside 1..64", top_k);
  if (!keep || !score) return fail(-10, "ssd_decode: NULL output");
  return hip_check(launch_ssd_decode(B, n, C, loc, cls, conf, nms_thr, top_k, keep, score, (hipStream_t)stream),
                   "ssd_decode");
}

// ---- landmark front end: top-1 decode + crop boxes, the banded accuracy (tpg_ssd.hip) and
// ToTensor (tpg_data.hip)
extern "C" int32_t tpg_ssd_landmarks(int32_t B, int32_t n, int32_t C, const float* loc, const float* cls, float conf,
                                     const float* scale, const int32_t* patch_wh, float* points, float* score,
                                     int32_t* anchor, int32_t* boxes, int32_t* status, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  int32_t rc = check_ssd(B, n, C, loc, cls, "ssd_landmarks");
  if (rc) return rc;
  if (!patch_wh || !points || !score || !anchor || !boxes || !status) return fail(-10, "ssd_landmarks: NULL pointer");
  if ((uintptr_t)scale % 4) return fail(-15, "ssd_landmarks: scale must be 4-byte aligned");
  for (int i = 0; i < 8; ++i)
    if (patch_wh[i] <= 0) return fail(-2, "ssd_landmarks: bad patch size");
  return hip_check(launch_ssd_landmarks(B, n, C, loc, cls, conf, scale, patch_wh, points, score, anchor, boxes, status,
                                        (hipStream_t)stream), "ssd_landmarks");
}

extern "C" int32_t tpg_landmark_accuracy(int32_t B, const float* pred, const float* truth, const int32_t* status,
                                         int32_t nbands, const float* thresholds, const float* weights, float* acc,
                                         tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  if (B < 1 || nbands < 1 || nbands > TPG_LM_MAX_BANDS)
    return fail(-2, "landmark_accuracy: B %d, nbands %d (1..%d)", B, nbands, TPG_LM_MAX_BANDS);
  if (!pred || !truth || !thresholds || !weights || !acc) return fail(-10, "landmark_accuracy: NULL pointer");
  for (int i = 0; i < nbands; ++i)
    if (!(thresholds[i] >= (i ? thresholds[i - 1] : 0.f)))
      return fail(-2, "landmark_accuracy: thresholds must ascend from 0 (band %d)", i);
  return hip_check(launch_landmark_accuracy(B, pred, truth, status, nbands, thresholds, weights, acc,
                                            (hipStream_t)stream), "landmark_accuracy");
}

extern "C" int32_t tpg_u8_to_unit(int32_t n, int32_t c, int32_t h, int32_t w, const uint8_t* img,
                                  const int64_t* img_stride, tpg_tensor out, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  // (h * w first: the product of three 31-bit sizes does not fit 64 bits)
  if (n < 1 || c < 1 || h < 1 || w < 1 || (int64_t)h * w > 0x7fffffffLL || (int64_t)h * w * n > 0x7fffffffLL)
    return fail(-2, "u8_to_unit: bad sizes %d x %d x %d x %d", n, c, h, w);
  if (!img || !img_stride || !out.data) return fail(-10, "u8_to_unit: NULL pointer");
  if (out.dtype != TPG_F32 && out.dtype != TPG_BF16 && out.dtype != TPG_F16)
    return fail(-11, "u8_to_unit: bad dtype %d", out.dtype);
  return hip_check(launch_u8_to_unit(n, c, h, w, img, img_stride, out, (hipStream_t)stream), "u8_to_unit");
}
