// The convolution planners: pure functions of (PlanCtx, descriptor, tensor layouts) that turn a
// tpg_conv_desc into finished launch plans.  tpg_plan_data.hip plans the forward and the input
// gradient, tpg_plan_wgrad.hip the weight gradient; tpg_capi.hip adds the data pointers and
// launches.  Host arithmetic only: the planner units make no device-runtime call, launch nothing,
// never touch the launch-group record, and from the kernel files call only the host predicates
// listed under one heading in tpg_internal.h.
#pragma once
#include "tpg_internal.h"
#include <string.h>
#include <algorithm>
#include <vector>

namespace tpg {

inline int esize(int dtype) { return dtype == TPG_F32 ? 4 : 2; }
inline bool half16(int dtype) { return dtype == TPG_BF16 || dtype == TPG_F16; }  // 16-bit MFMA operands
inline int64_t rup(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int pmod(int a, int m) { return ((a % m) + m) % m; }

// Everything a plan depends on besides the geometry and the tensors' layout, read once per
// entry point: the planners take it as an argument and read no global.
struct PlanCtx {
  int share;  // share of the chip the op plans its grid for: 1, or 4 with TPG_FLAG_CONCURRENT (the
              // op runs beside other streams' work, e.g. the four local pathways: fewer K / pixel
              // splits, since the other streams fill the CUs a split would; 1/2 .. 1/8 measured
              // within run-to-run spread, profiles/r02c/share)
  int ks;     // forced k-step split of the forward / input-gradient launches (desc.data_ksplit; 0 = planner)
  int algo;   // kernel of the small-map multi-tap forward / input-gradient plans (desc.data_algo; 0 = rule)
  bool det;   // tpg_set_deterministic
};
PlanCtx plan_ctx(const tpg_conv_desc* d);

// ------------------------------------------------------------------ problem plans --
// (the argument blocks' data pointers, strides and vector flags stay zero in a plan: run_data
// fills copies)
struct Prob {
  IgemmArgs a;
  PackArgs pk;
  int cfg = 0;
  size_t wp_bytes = 0, sk_bytes = 0;
  bool halo = false;          // run on the halo-tiled direct-conv kernel (h.pw > 0: the pointwise one)
  HaloArgs h;
  int hcfg = -1, hbm = 0;     // halo config id and rows per block
  size_t g_wp = 0, g_sk = 0;  // generic-kernel sizes: tensors the halo kernel cannot read fall back to it
  size_t wp_off = 0;          // weight region [wp_off, wp_off + region()) of the workspace / packed image
  size_t region() const { return std::max(wp_bytes, g_wp); }
  Prob() {
    memset(&a, 0, sizeof(a));
    memset(&pk, 0, sizeof(pk));
    memset(&h, 0, sizeof(h));
  }
};

// The tensors of a forward / input-gradient call as the plan sees them: strides, dtypes and
// pointer alignment, never the data.  A = x or the incoming gradient, Y = y or dx; M, G: the
// saved output and the g buffer of the masked input-gradient mode; X: the conv's input when
// desc.in_act rides the epilogues.  All null: the 16-byte aligned dense tensors the workspace
// and pre-pack queries assume.
struct DataLayouts {
  const tpg_tensor *A = nullptr, *Y = nullptr, *M = nullptr, *G = nullptr, *X = nullptr;
  bool residual = false, packed = false;
};

// One finished plan of tpg_conv2d_fwd / _bwd_data / the masked attempt of tpg_conv2d_bwd.
struct DataPlan {
  std::vector<Prob> v;
  tpg_conv_desc d;
  bool fwd = true, comp = false, refl = false, masked = false, xa = false, packed = false;
  int bias_mod = 0;
  size_t tmp_bytes = 0;  // reflect: the padded input's gradient, at the start of the workspace
  size_t sk_off = 0;     // split-K slices (shared by the problems, which run one after another)
  size_t need = 0;       // bytes of workspace the launch uses
};

// (the weight regions alone: the packed image of tpg_conv2d_packed_bytes / _pack_jobs)
inline size_t packed_bytes(const DataPlan& p) { return p.sk_off; }

// ---- weight-gradient plans: kernel family, tile, pixel split and every launch argument that
// needs no data pointer.
struct WgradPlan {
  int kernel;       // TPG_WGRAD_*
  int cfg, bm, bn, tiles;
  bool sums_bias;   // the launch adds dbias when given one
  bool p_is_x;      // iteration-grid operand P: x (ConvTranspose2d) or g
  WgradArgs a;      // generic and flat kernels
  WgradRHArgs rh;   // row- and image-halo kernels
};

// tpg_plan_data.hip
int32_t check_desc(const tpg_conv_desc* d);
int32_t check_tensor(const tpg_tensor& t, int dtype, const char* name);
bool vec_ok(const tpg_tensor& t, int dtype);
bool big_taps(const tpg_conv_desc* d);
bool composite(const tpg_conv_desc* d, const tpg_tensor* in, const tpg_tensor* out);
void plan_probs(const PlanCtx& cx, const tpg_conv_desc* d, bool fwd, bool comp, DataPlan* p);
size_t data_workspace(const PlanCtx& cx, const tpg_conv_desc* d, bool fwd);
int32_t plan_data(const PlanCtx& cx, const tpg_conv_desc* d, int32_t op, const DataLayouts& L, size_t ws_bytes,
                  DataPlan* p);
// tpg_plan_wgrad.hip
int32_t plan_bwd_filter(const tpg_conv_desc* d, const tpg_tensor& x, const tpg_tensor& g, const tpg_tensor& dw,
                        WgradPlan* p);

}  // namespace tpg
